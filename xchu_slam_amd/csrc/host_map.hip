// host_map.hip — the keyframe store and the global map on a ctx (pgo_node's SaveMap :620-653, PublishPoseAndFrame
// :744-812, LoopFindNearKeyframesCloud :530-554): ndt_map_*.  The keyframes live in one device arena; a build stacks any
// selection of them under per-keyframe poses in one k_map_stack launch and runs the ctx's pcl::VoxelGrid behind it.
// Everything goes to the ctx stream.
#include "ndt_host.h"

struct ndt_map {
    ndt_ctx* c = nullptr;
    DevBuf<float4> arena;               // every keyframe's points, in the order they were added (arena.cap: room, in points)
    size_t used = 0;                    // points held
    std::vector<long long> off, count;  // per keyframe: first point in the arena, points
    DevBuf<float4> stack;               // the stacked cloud of a build with a leaf (VoxelGrid's input)
    DevBuf<float4> result;              // the map's own result buffer (builds with d_out4 NULL)
    size_t result_n = 0;
    bool has_result = false;
    DevBuf<char> d_tab;                 // the build's table: prefix, arena offsets, poses
    Pinned<char[]> h_tab;               // its pinned staging copy (a build ends synchronised: free to rewrite)
    size_t h_tab_cap = 0;
    int geom[4] = {0, kBlock, kMapPointsPerWg, 0};
};

// Room for `need` points, contents kept bit for bit: at least double the room, the held points moved device to device
// on the ctx stream.  A growth that fails leaves the arena as it was.  The stream is synchronised before the old block
// is released (queued launches and the copy read it); pointers from ndt_map_keyframe die here.
static ndt_status map_reserve(ndt_map* m, size_t need) {
    ndt_ctx* c = m->c;
    if (need <= m->arena.cap) return NDT_OK;
    const size_t cap = std::max(need, m->arena.cap * 2);
    DevBuf<float4> blk;  // the new block; after the swap below the previous one, released on return
    if (hipMalloc(&blk.p, cap * sizeof(float4)) != hipSuccess) {
        blk.p = nullptr;
        return fail(c, NDT_ENOMEM, "keyframe arena allocation failed");
    }
    blk.cap = cap;
    TRY(copy16(c, c->stream.get(), blk.p, m->arena.p, m->used * sizeof(float4)));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    std::swap(m->arena, blk);
    return NDT_OK;
}

static ndt_status map_push(ndt_map* m, size_t n, int* index) {
    if (index) *index = (int)m->count.size();
    m->off.push_back((long long)m->used);
    m->count.push_back((long long)n);
    m->used += n;
    return NDT_OK;
}

static ndt_status map_can_add(ndt_map* m, size_t n) {
    if (n > 0x7fffffffULL) return fail(m->c, NDT_EINVAL, "cloud too large");
    if (m->count.size() >= 0x7fffffffULL) return fail(m->c, NDT_EINVAL, "too many keyframes");
    return NDT_OK;
}

extern "C" {

ndt_status ndt_map_create(ndt_ctx* c, ndt_map** out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    *out = nullptr;
    ndt_map* m = new ndt_map();
    m->c = c;
    *out = m;
    return NDT_OK;
}

void ndt_map_destroy(ndt_map* m) {
    if (!m) return;
    drain_for_destroy(m->c);
    delete m;
}

int ndt_map_size(const ndt_map* m) { return m ? (int)m->count.size() : -1; }

ndt_status ndt_map_points(const ndt_map* m, long long* points) {
    if (!m) return NDT_EINVAL;
    if (!points) return fail(m->c, NDT_EINVAL, "null argument");
    *points = (long long)m->used;
    return NDT_OK;
}

ndt_status ndt_map_capacity(const ndt_map* m, long long* points) {
    if (!m) return NDT_EINVAL;
    if (!points) return fail(m->c, NDT_EINVAL, "null argument");
    *points = (long long)m->arena.cap;
    return NDT_OK;
}

ndt_status ndt_map_reserve(ndt_map* m, long long points) {
    if (!m) return NDT_EINVAL;
    if (points < 0) return fail(m->c, NDT_EINVAL, "negative reserve");
    TRY(set_dev(m->c));
    return map_reserve(m, (size_t)points);
}

ndt_status ndt_map_add(ndt_map* m, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset, int* index) {
    if (!m) return NDT_EINVAL;
    ndt_ctx* c = m->c;
    if (n && (!xyzi || !xyzi_layout_ok(stride_bytes, intensity_offset))) return fail(c, NDT_EINVAL, "bad cloud arguments");
    TRY(map_can_add(m, n));
    TRY(set_dev(c));
    if (n) {
        TRY(map_reserve(m, m->used + n));
        const std::vector<float> tmp = pack_cloud4(xyzi, n, stride_bytes, intensity_offset);
        HIPCHK(c, hipMemcpyAsync(m->arena.p + m->used, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));  // tmp goes on return
    }
    return map_push(m, n, index);
}

ndt_status ndt_map_add_device(ndt_map* m, const float* d_xyzi4, size_t n, int* index) {
    if (!m) return NDT_EINVAL;
    ndt_ctx* c = m->c;
    if (n && !d_xyzi4) return fail(c, NDT_EINVAL, "null argument");
    TRY(map_can_add(m, n));
    TRY(set_dev(c));
    if (n) {
        TRY(map_reserve(m, m->used + n));
        TRY(copy16(c, c->stream.get(), m->arena.p + m->used, d_xyzi4, n * sizeof(float4)));
    }
    return map_push(m, n, index);
}

ndt_status ndt_map_keyframe(ndt_map* m, int index, const float** d_xyzi4, size_t* n) {
    if (!m) return NDT_EINVAL;
    if (index < 0 || (size_t)index >= m->count.size()) return fail(m->c, NDT_EINVAL, "keyframe index out of range");
    if (d_xyzi4) *d_xyzi4 = reinterpret_cast<const float*>(m->arena.p + m->off[(size_t)index]);
    if (n) *n = (size_t)m->count[(size_t)index];
    return NDT_OK;
}

ndt_status ndt_map_get_keyframe(ndt_map* m, int index, float* out4, size_t cap, size_t* n_out) {
    if (!m) return NDT_EINVAL;
    ndt_ctx* c = m->c;
    if (index < 0 || (size_t)index >= m->count.size()) return fail(c, NDT_EINVAL, "keyframe index out of range");
    const size_t n = (size_t)m->count[(size_t)index], k = std::min(cap, n);
    if (k && !out4) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    if (k) HIPCHK(c, hipMemcpy(out4, m->arena.p + m->off[(size_t)index], k * sizeof(float4), hipMemcpyDeviceToHost));
    if (n_out) *n_out = n;
    return NDT_OK;
}

ndt_status ndt_map_count(ndt_map* m, const int* index, int n_sel, long long* total) {
    if (!m) return NDT_EINVAL;
    if (n_sel < 0 || !total) return fail(m->c, NDT_EINVAL, "bad selection arguments");
    std::vector<long long> prefix;
    if (!map_selection_prefix(m->count, index, n_sel, prefix)) return fail(m->c, NDT_EINVAL, "keyframe index out of range");
    *total = prefix[(size_t)n_sel];
    return NDT_OK;
}

ndt_status ndt_map_build(ndt_map* m, const int* index, const float* T16, int n_sel, float leaf, float* d_out4, size_t cap, size_t* n_out) {
    if (!m) return NDT_EINVAL;
    ndt_ctx* c = m->c;
    if (n_sel < 0 || !n_out || !(leaf >= 0.f)) return fail(c, NDT_EINVAL, "bad build arguments");
    if (n_sel > 0 && !T16) return fail(c, NDT_EINVAL, "null poses");
    std::vector<long long> prefix;
    if (!map_selection_prefix(m->count, index, n_sel, prefix)) return fail(c, NDT_EINVAL, "keyframe index out of range");
    const long long total = prefix[(size_t)n_sel];
    if (total > 0x7fffffffLL) return fail(c, NDT_EINVAL, "selection exceeds 2^31 - 1 points");
    if (d_out4 && cap < (size_t)total) return fail(c, NDT_EINVAL, "output buffer too small for the stacked selection");
    TRY(set_dev(c));
    *n_out = 0;
    m->geom[0] = 0;
    m->geom[3] = n_sel;
    if (total == 0) {
        if (!d_out4) { m->result_n = 0; m->has_result = true; }
        return NDT_OK;
    }
    if (!d_out4) {
        m->has_result = false;
        TRY(ensure(c, m->result, (size_t)total));
    }
    float4* dest = d_out4 ? reinterpret_cast<float4*>(d_out4) : m->result.p;
    float4* stacked = dest;
    if (leaf > 0.f) {
        TRY(ensure(c, m->stack, (size_t)total));
        stacked = m->stack.p;
    }
    // the table: prefix (n_sel + 1 ints, padded to 8 bytes), each segment's arena offset, each segment's pose
    const size_t ns = (size_t)n_sel;
    const size_t o_off = ((ns + 1) * sizeof(int) + 7) / 8 * 8, o_T = o_off + ns * sizeof(long long), bytes = o_T + ns * sizeof(Mat4f);
    if (bytes > m->h_tab_cap) {
        const size_t want = std::max(bytes, m->h_tab_cap * 2);
        Pinned<char[]> p;
        TRY(make_pinned(c, p, want, hipHostMallocDefault));
        m->h_tab = std::move(p);
        m->h_tab_cap = want;
    }
    TRY(ensure(c, m->d_tab, bytes));
    char* h = m->h_tab.get();
    int* h_prefix = reinterpret_cast<int*>(h);
    long long* h_off = reinterpret_cast<long long*>(h + o_off);
    for (size_t k = 0; k <= ns; ++k) h_prefix[k] = (int)prefix[k];
    for (size_t k = 0; k < ns; ++k) h_off[k] = m->off[(size_t)(index ? index[k] : (int)k)];
    std::memcpy(h + o_T, T16, ns * sizeof(Mat4f));
    HIPCHK(c, hipMemcpyAsync(m->d_tab.p, h, bytes, hipMemcpyHostToDevice, c->stream.get()));
    const int nb = map_stack_blocks(total);
    m->geom[0] = nb;
    hipLaunchKernelGGL(k_map_stack, dim3(nb), dim3(kBlock), 0, c->stream.get(), m->arena.p, reinterpret_cast<const int*>(m->d_tab.p),
                       reinterpret_cast<const long long*>(m->d_tab.p + o_off), reinterpret_cast<const Mat4f*>(m->d_tab.p + o_T), n_sel,
                       (int)total, kMapPointsPerWg, stacked);
    HIPCHK(c, hipGetLastError());
    ndt_status rs = NDT_OK;
    if (leaf > 0.f) {
        // NDT_EOVERFLOW: the leaf overflowed pcl::VoxelGrid's index range, dest holds the stacked cloud itself
        rs = voxel_downsample_dev(c, stacked, (size_t)total, leaf, dest, n_out);
        if (rs != NDT_OK && rs != NDT_EOVERFLOW) return rs;
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
        *n_out = (size_t)total;
    }
    if (!d_out4) { m->result_n = *n_out; m->has_result = true; }
    return rs;
}

ndt_status ndt_map_result(ndt_map* m, const float** d_out4, size_t* n) {
    if (!m) return NDT_EINVAL;
    if (!m->has_result) return fail(m->c, NDT_EINVAL, "no build into the map's own buffer yet");
    if (d_out4) *d_out4 = reinterpret_cast<const float*>(m->result.p);
    if (n) *n = m->result_n;
    return NDT_OK;
}

ndt_status ndt_map_get(ndt_map* m, float* out4, size_t cap, size_t* n_out) {
    if (!m) return NDT_EINVAL;
    ndt_ctx* c = m->c;
    if (!m->has_result) return fail(c, NDT_EINVAL, "no build into the map's own buffer yet");
    const size_t k = std::min(cap, m->result_n);
    if (k && !out4) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    if (k) HIPCHK(c, hipMemcpy(out4, m->result.p, k * sizeof(float4), hipMemcpyDeviceToHost));
    if (n_out) *n_out = m->result_n;
    return NDT_OK;
}

ndt_status ndt_map_geometry(ndt_map* m, int out[4]) {
    if (!m) return NDT_EINVAL;
    if (!out) return fail(m->c, NDT_EINVAL, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = m->geom[k];
    return NDT_OK;
}

}  // extern "C"
