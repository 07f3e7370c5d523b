// host_sc.hip — Scan Context on a ctx (SCManager of Scancontext.{h,cpp}, pgo_node's loop detector): ndt_sc_*.
// The database lives on the device; every launch goes to the ctx stream and only result records come back.
#include "ndt_host.h"

struct ndt_sc {
    ndt_ctx* c = nullptr;
    ndt_sc_params prm{};
    int size = 0;
    SlotArrays mem;                 // the database's arrays
    ScDb db{nullptr, nullptr, nullptr, nullptr};
    DevBuf<unsigned> bins;          // k_sc_make's merged bin images of the descriptor being added
    DevBuf<float4> pts;             // ndt_sc_add's upload
    DevBuf<int> d_query, d_nsearch; // ndt_sc_detect_batch's arguments
    DevBuf<ndt_sc_result> d_res;
    // detectLoopClosureID's state: the period counter and the size of the searchable ring-key prefix
    long long counter = 0;
    int searchable = 0;
};

static bool sc_valid_params(const ndt_sc_params* p) {
    return p && p->num_candidates >= 1 && p->num_candidates <= kScMaxCand && p->search_ratio >= 0.0 && p->search_ratio <= 1.0 &&
           p->num_exclude_recent >= 0 && p->tree_making_period >= 1 && !std::isnan(p->dist_thres);
}

namespace ndt::host {

// Room for `need` slots in a database that stores `size`, contents kept: capacity 64, then doubling; one device block,
// each array (slot_bytes[k] per slot) at a 256-byte boundary of it; the stored slots move device to device.  A growth
// that fails leaves the database as it was.  The stream is synchronised before the copies (launches queued on it
// may still write the old block) and again before the old block is released.
ndt_status reserve_slots(ndt_ctx* c, SlotArrays& a, size_t size, size_t need, std::initializer_list<size_t> slot_bytes, const char* what) {
    if (need <= a.cap) return NDT_OK;
    const size_t cap = std::max<size_t>(std::max<size_t>(need, 64), a.cap * 2);
    std::vector<size_t> off;
    size_t total = 0;
    for (size_t b : slot_bytes) {
        off.push_back(total);
        total += (cap * b + 255) / 256 * 256;
    }
    DevBuf<char> blk;  // the new block; after the swap below the previous one, released on return
    if (hipMalloc(&blk.p, total) != hipSuccess) {
        blk.p = nullptr;
        return fail(c, NDT_ENOMEM, std::string(what) + " database allocation failed");
    }
    blk.cap = total;
    hipError_t e = hipStreamSynchronize(c->stream.get());
    size_t k = 0;
    for (size_t b : slot_bytes) {
        if (e == hipSuccess && size) e = hipMemcpyAsync(blk.p + off[k], a.arr[k], size * b, hipMemcpyDeviceToDevice, c->stream.get());
        ++k;
    }
    if (e == hipSuccess && size) e = hipStreamSynchronize(c->stream.get());
    if (e != hipSuccess) return fail(c, NDT_EDEVICE, std::string(what) + " database growth: " + hipGetErrorString(e));
    std::swap(a.block, blk);
    a.arr.clear();
    for (size_t o : off) a.arr.push_back(a.block.p + o);
    a.cap = cap;
    return NDT_OK;
}

}  // namespace ndt::host

static ndt_status sc_reserve(ndt_sc* sc, size_t need) {
    TRY(reserve_slots(sc->c, sc->mem, (size_t)sc->size, need,
                      {kScBins * sizeof(double), kScRings * sizeof(float), kScSectors * sizeof(double), kScSectors * sizeof(double)}, "Scan Context"));
    sc->db = ScDb{sc->mem.at<double>(0), sc->mem.at<float>(1), sc->mem.at<double>(2), sc->mem.at<double>(3)};
    return NDT_OK;
}

static ndt_status sc_add_points(ndt_sc* sc, const float4* d_pts, size_t n, int* index) {
    ndt_ctx* c = sc->c;
    if (n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "cloud too large");
    TRY(sc_reserve(sc, (size_t)sc->size + 1));
    TRY(ensure(c, sc->bins, kScBins));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)sc->bins.p, (int)sc_image(kScNoPoint), kScBins, c->stream.get()));
    if (n) {
        const int nb = std::min(ceil_div((long long)n, kScBlock * kScMakePerThread), kScMakeMaxBlocks);
        hipLaunchKernelGGL(k_sc_make, dim3(nb), dim3(kScBlock), 0, c->stream.get(), d_pts, (int)n, sc->bins.p);
    }
    hipLaunchKernelGGL(k_sc_finalize, dim3(1), dim3(kScBlock), 0, c->stream.get(), sc->bins.p, sc->db, sc->size);
    HIPCHK(c, hipGetLastError());
    if (index) *index = sc->size;
    ++sc->size;
    return NDT_OK;
}

// one k_sc_detect launch over n queries (device arrays, or the single q0 / ns0), records copied to out; synchronises
static ndt_status sc_run(ndt_sc* sc, const int* d_query, const int* d_nsearch, int q0, int ns0, int pair_j, int n, ndt_sc_result* out) {
    ndt_ctx* c = sc->c;
    TRY(ensure(c, sc->d_res, (size_t)n));
    ScDetectArgs a;
    a.num_candidates = sc->prm.num_candidates;
    a.radius = (int)std::round(0.5 * sc->prm.search_ratio * kScSectors);
    a.dist_thres = sc->prm.dist_thres;
    a.pair_j = pair_j;
    hipLaunchKernelGGL(k_sc_detect, dim3(n), dim3(kScBlock), 0, c->stream.get(), sc->db, d_query, d_nsearch, q0, ns0, a, sc->d_res.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, sc->d_res.p, (size_t)n * sizeof(ndt_sc_result), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    return NDT_OK;
}

extern "C" {

// The constants of Scancontext.h:83-104 (SC_DIST_THRES as pgo_node's build has it)
ndt_status ndt_sc_default_params(ndt_sc_params* out) {
    if (!out) return NDT_EINVAL;
    out->dist_thres = 0.2;
    out->num_exclude_recent = 30;
    out->num_candidates = 3;
    out->tree_making_period = 30;
    out->search_ratio = 0.1;
    return NDT_OK;
}

ndt_status ndt_sc_create(ndt_ctx* c, const ndt_sc_params* prm, ndt_sc** out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    *out = nullptr;
    ndt_sc_params p;
    (void)ndt_sc_default_params(&p);
    if (prm) p = *prm;
    if (!sc_valid_params(&p)) return fail(c, NDT_EINVAL, "invalid Scan Context params");
    ndt_sc* sc = new ndt_sc();
    sc->c = c;
    sc->prm = p;
    *out = sc;
    return NDT_OK;
}

void ndt_sc_destroy(ndt_sc* sc) {
    if (!sc) return;
    drain_for_destroy(sc->c);
    delete sc;
}

ndt_status ndt_sc_set_params(ndt_sc* sc, const ndt_sc_params* prm) {
    if (!sc) return NDT_EINVAL;
    if (!sc_valid_params(prm)) return fail(sc->c, NDT_EINVAL, "invalid Scan Context params");
    sc->prm = *prm;
    return NDT_OK;
}

int ndt_sc_size(const ndt_sc* sc) { return sc ? sc->size : -1; }

ndt_status ndt_sc_add_device(ndt_sc* sc, const float* d_xyz4, size_t n, int* index) {
    if (!sc) return NDT_EINVAL;
    if (n && !d_xyz4) return fail(sc->c, NDT_EINVAL, "null argument");
    TRY(set_dev(sc->c));
    return sc_add_points(sc, reinterpret_cast<const float4*>(d_xyz4), n, index);
}

ndt_status ndt_sc_add(ndt_sc* sc, const float* xyz, size_t n, size_t stride_bytes, int* index) {
    if (!sc) return NDT_EINVAL;
    if (n && (!xyz || stride_bytes < 12)) return fail(sc->c, NDT_EINVAL, "bad cloud arguments");
    TRY(set_dev(sc->c));
    TRY(upload_points(sc->c, sc->pts, xyz, n, stride_bytes));  // synchronises: the previous add has read sc->pts
    return sc_add_points(sc, sc->pts.p, n, index);
}

ndt_status ndt_sc_add_descriptor(ndt_sc* sc, const double desc[1200], int* index) {
    if (!sc) return NDT_EINVAL;
    ndt_ctx* c = sc->c;
    if (!desc) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    TRY(sc_reserve(sc, (size_t)sc->size + 1));
    HIPCHK(c, hipMemcpyAsync(sc->db.desc + (size_t)sc->size * kScBins, desc, kScBins * sizeof(double), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));  // the caller's array is free on return
    hipLaunchKernelGGL(k_sc_finalize, dim3(1), dim3(kScBlock), 0, c->stream.get(), (const unsigned*)nullptr, sc->db, sc->size);
    HIPCHK(c, hipGetLastError());
    if (index) *index = sc->size;
    ++sc->size;
    return NDT_OK;
}

ndt_status ndt_sc_detect(ndt_sc* sc, ndt_sc_result* out) {
    if (!sc) return NDT_EINVAL;
    ndt_ctx* c = sc->c;
    if (!out) return fail(c, NDT_EINVAL, "null argument");
    if (sc->size == 0) return fail(c, NDT_EINVAL, "no descriptor stored");
    TRY(set_dev(c));
    int ns = 0;
    if (sc->size >= sc->prm.num_exclude_recent + 1) {
        if (sc->counter % sc->prm.tree_making_period == 0) sc->searchable = sc->size - sc->prm.num_exclude_recent;
        ++sc->counter;
        ns = sc->searchable;
    }
    return sc_run(sc, nullptr, nullptr, sc->size - 1, ns, -1, 1, out);
}

ndt_status ndt_sc_detect_batch(ndt_sc* sc, const int* query, const int* n_search, int n, ndt_sc_result* out) {
    if (!sc) return NDT_EINVAL;
    ndt_ctx* c = sc->c;
    if (n < 0 || (n && (!query || !n_search || !out))) return fail(c, NDT_EINVAL, "bad batch arguments");
    if (n == 0) return NDT_OK;
    for (int i = 0; i < n; ++i)
        if (query[i] < 0 || query[i] >= sc->size || n_search[i] > sc->size) return fail(c, NDT_EINVAL, "query or search range outside the stored descriptors");
    TRY(set_dev(c));
    TRY(ensure(c, sc->d_query, (size_t)n));
    TRY(ensure(c, sc->d_nsearch, (size_t)n));
    HIPCHK(c, hipMemcpyAsync(sc->d_query.p, query, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipMemcpyAsync(sc->d_nsearch.p, n_search, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream.get()));
    return sc_run(sc, sc->d_query.p, sc->d_nsearch.p, 0, 0, -1, n, out);
}

ndt_status ndt_sc_distance(ndt_sc* sc, int i, int j, double* dist, int* shift) {
    if (!sc) return NDT_EINVAL;
    ndt_ctx* c = sc->c;
    if (i < 0 || j < 0 || i >= sc->size || j >= sc->size) return fail(c, NDT_EINVAL, "descriptor index out of range");
    TRY(set_dev(c));
    ndt_sc_result r;
    TRY(sc_run(sc, nullptr, nullptr, i, 0, j, 1, &r));
    if (dist) *dist = r.cand_dist[0];
    if (shift) *shift = r.cand_shift[0];
    return NDT_OK;
}

ndt_status ndt_sc_get(ndt_sc* sc, int index, double* desc, float* ringkey, double* sectorkey) {
    if (!sc) return NDT_EINVAL;
    ndt_ctx* c = sc->c;
    if (index < 0 || index >= sc->size) return fail(c, NDT_EINVAL, "descriptor index out of range");
    TRY(set_dev(c));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    const size_t k = (size_t)index;
    if (desc) HIPCHK(c, hipMemcpy(desc, sc->db.desc + k * kScBins, kScBins * sizeof(double), hipMemcpyDeviceToHost));
    if (ringkey) HIPCHK(c, hipMemcpy(ringkey, sc->db.ringkey + k * kScRings, kScRings * sizeof(float), hipMemcpyDeviceToHost));
    if (sectorkey) HIPCHK(c, hipMemcpy(sectorkey, sc->db.sectorkey + k * kScSectors, kScSectors * sizeof(double), hipMemcpyDeviceToHost));
    return NDT_OK;
}

}  // extern "C"
