// host_ground.hip — filter_node's ground detection over a scan (CloudFilter::DetectPlane, filter_node.cpp:103-216):
// ndt_ground_*, ndt_filter_ground_scan.  Kernels in ground.hip; semantics in DESIGN.md §2 "Ground".
//
// One detect is: tilt, clip flags, compaction (one read of the clipped count, which sizes the neighbour index's sort),
// index build, k_ground_normals, compaction (its count stays on the device), tilt back, then chains of kGroundChain x
// (k_ground_sample, k_ground_score) + k_ground_finish and one read of the state per chain.  The first chain ends almost
// every scan (kGroundBatch, ndt_ground.h); a launch behind the end of the loop returns at its first load.  The
// compactions are host_front_end.hip's enqueue_compact4 (with compact4_count where the host reads the count), the
// clouds' VoxelGrid its voxel_downsample_dev.
#include "ndt_host.h"

namespace {

constexpr unsigned kGroundSeed = 12345u;  // SampleConsensusModel's rng_alg_ seed, set anew for every scan's model

ndt_status ground_params_ok(ndt_ctx* c, const ndt_ground_params& p) {
    if (p.struct_size != sizeof(ndt_ground_params)) return fail(c, NDT_EINVAL, "ndt_ground_params: struct_size is not this library's");
    if (!std::isfinite(p.tilt_deg) || !std::isfinite(p.sensor_height) || !std::isfinite(p.height_clip_range) || p.floor_pts_thresh < 3 ||
        !std::isfinite(p.floor_normal_thresh) || !std::isfinite(p.normal_filter_thresh) || p.normal_k < 1 || p.normal_k > kGroundMaxK ||
        !(p.ransac_threshold > 0.0) || !(p.ransac_probability > 0.0 && p.ransac_probability < 1.0) || p.ransac_max_iterations < 1 ||
        p.ransac_max_iterations > kGroundMaxIterations || !(p.cloud_leaf >= 0.f))
        return fail(c, NDT_EINVAL, "invalid ground params");
    return NDT_OK;
}

// what every detect needs from the first one on, made together
ndt_status ground_buffers(ndt_ctx* c) {
    GroundRun& g = c->ground;
    if (g.h_state) return NDT_OK;
    DevBuf<GridHeader> hdr, ixh;
    DevBuf<GroundState> st;
    DevBuf<double> part;
    DevBuf<unsigned> ticket;
    Pinned<GroundState[]> hs;
    Pinned<int[]> hw;
    if (ensure(c, hdr, 1) != NDT_OK || ensure(c, ixh, 1) != NDT_OK || ensure(c, st, 1) != NDT_OK ||
        ensure(c, part, (size_t)kGroundBatch * kGroundScoreMaxBlocks) != NDT_OK || ensure(c, ticket, 64) != NDT_OK ||
        make_pinned(c, hs, 2, hipHostMallocDefault) != NDT_OK || make_pinned(c, hw, 4, hipHostMallocDefault) != NDT_OK)
        return fail(c, NDT_ENOMEM, "ground state allocation failed");
    HIPCHK(c, hipMemsetAsync(hdr.p, 0, sizeof(GridHeader), c->stream.get()));
    HIPCHK(c, hipMemsetAsync(ticket.p, 0, ticket.cap * sizeof(unsigned), c->stream.get()));
    g.d_hdr = std::move(hdr);
    g.ix.hdr = std::move(ixh);
    g.d_state = std::move(st);
    g.part = std::move(part);
    g.ticket = std::move(ticket);
    g.h_words = std::move(hw);
    g.h_state = std::move(hs);
    return NDT_OK;
}

// the generator's first `words` outputs on the device (a power of two), and a hash of twice as many slots
ndt_status ground_table(ndt_ctx* c, size_t words) {
    GroundRun& g = c->ground;
    if (g.table_words >= words) return NDT_OK;
    const std::vector<uint32_t> v = mt19937_stream(kGroundSeed, words);
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));  // nothing queued reads the old table any more
    TRY(ensure(c, g.table, words));
    TRY(ensure(c, g.hash, 2 * words));
    HIPCHK(c, hipMemcpy(g.table.p, v.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
    g.table_words = words;
    return NDT_OK;
}

// AngleAxisf(tilt_deg * pi / 180, UnitY) as a Matrix4f, and its inverse: the rotation transposed
void tilt_matrices(double tilt_deg, Mat4f* T, Mat4f* Tinv) {
    float R[9];
    angle_axis_f((float)(tilt_deg * M_PI / 180.0f), 1, R);
    for (int k = 0; k < 16; ++k) T->m[k] = Tinv->m[k] = (k % 5 == 0) ? 1.f : 0.f;
    for (int col = 0; col < 3; ++col)
        for (int row = 0; row < 3; ++row) {
            T->m[4 * col + row] = R[row + 3 * col];
            Tinv->m[4 * row + col] = R[row + 3 * col];
        }
}

// words of the first table a context uploads; NDT_GROUND_STREAM (a power of two, 16 .. kGroundStreamWords) shortens it
// for runs that exercise the continuation
size_t first_table_words() {
    size_t words = kGroundStreamWords;
    if (const char* e = std::getenv("NDT_GROUND_STREAM")) {
        const long v = std::atol(e);
        if (v >= 16 && v <= kGroundStreamWords && (v & (v - 1)) == 0) words = (size_t)v;
    }
    return words;
}

// the scan's RANSAC from its first sample: the state h_state[1] uploaded, the hypotheses and the hash cleared, chains of
// launches until the loop has ended
ndt_status ground_ransac(ndt_ctx* c, int m) {
    GroundRun& g = c->ground;
    hipStream_t st = c->stream.get();
    HIPCHK(c, hipMemsetAsync(g.tri.p, 0xff, g.hyp_cap * sizeof(int4), st));  // every sample GROUND_SAMPLE_NONE
    HIPCHK(c, hipMemsetAsync(g.hash.p, 0xff, 2 * g.table_words * sizeof(int2), st));
    if (!g.inject.empty()) HIPCHK(c, hipMemcpyAsync(g.tri.p, g.inject.data(), g.inject.size() * sizeof(int), hipMemcpyHostToDevice, st));
    const int nbs = grid_for(m, kGroundBlock, kGroundScoreMaxBlocks), nbf = grid_for(m, kGroundBlock, 2048);
    const int max_batches = (int)(g.hyp_cap / kGroundBatch);
    bool done = false;
    for (int batch = 0; !done && batch < max_batches;) {
        for (int b = 0; b < kGroundChain && batch < max_batches; ++b, ++batch) {
            hipLaunchKernelGGL(k_ground_sample, dim3(1), dim3(64), 0, st, g.nrm.p, g.d_state.p, batch, g.table.p, g.hash.p, g.tri.p);
            hipLaunchKernelGGL(k_ground_score, dim3(nbs), dim3(kGroundBlock), 0, st, g.nrm.p, g.d_state.p, batch, g.tri.p, g.coef.p,
                               g.stat.p, g.cnt.p, g.part.p, g.ticket.p);
        }
        hipLaunchKernelGGL(k_ground_finish, dim3(nbf), dim3(kGroundBlock), 0, st, g.nrm.p, g.nrm_org.p, m, g.d_state.p, g.tri.p, g.coef.p,
                           g.gflag.p, g.mark.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&g.h_words[2], &g.d_hdr.p->pad[0], sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&g.h_words[3], &g.ix.hdr.p->pad[0], sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&g.h_state[0], g.d_state.p, sizeof(GroundState), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        done = g.h_state[0].done != 0;
    }
    if (!done) return fail(c, NDT_EDEVICE, "ground: the RANSAC loop did not end within its hypotheses");
    return NDT_OK;
}

ndt_status ground_detect_dev(ndt_ctx* c, const ndt_ground_params* prm, const float4* d_in, size_t n, ndt_ground_result* out) {
    if (!out || out->struct_size != sizeof(ndt_ground_result)) return fail(c, NDT_EINVAL, "ndt_ground_result: struct_size is not this library's");
    ndt_ground_params p;
    p.struct_size = sizeof(p);
    (void)ndt_ground_default_params(&p);
    if (prm) p = *prm;
    TRY(ground_params_ok(c, p));
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an asynchronous align is in flight (ndt_align_wait first)");
    TRY(ground_buffers(c));
    GroundRun& g = c->ground;
    hipStream_t st = c->stream.get();
    g.valid = false;
    ndt_ground_result r{};
    r.struct_size = sizeof(r);
    r.n_input = (int)n;
    r.reason = NDT_GROUND_TOO_FEW_POINTS;
    r.winner[0] = r.winner[1] = r.winner[2] = -1;
    r.k = 1.0;
    g.prm = p;
    g.n_in = (int)n;
    g.n_clip = 0;
    auto leave = [&]() {
        g.res = r;
        g.valid = true;
        *out = r;
        return NDT_OK;
    };
    if (n == 0) return leave();
    const int N = (int)n;
    TRY(ensure(c, g.in, n)); TRY(ensure(c, g.tilted, n)); TRY(ensure(c, g.clip, n)); TRY(ensure(c, g.nrm_t, n)); TRY(ensure(c, g.nrm, n));
    TRY(ensure(c, g.normal4, n)); TRY(ensure(c, g.cloud, n)); TRY(ensure(c, g.flags, n)); TRY(ensure(c, g.idx, n));
    TRY(ensure(c, g.clip_org, n)); TRY(ensure(c, g.nrm_org, n)); TRY(ensure(c, g.nbr, n * (size_t)p.normal_k));
    TRY(ensure(c, g.gflag, n)); TRY(ensure(c, g.mark, n));
    if (d_in != g.in.p) HIPCHK(c, hipMemcpyAsync(g.in.p, d_in, n * sizeof(float4), hipMemcpyDeviceToDevice, st));
    // ---- a. tilt, b. height clip (filter_node.cpp:106-115)
    Mat4f T, Tinv;
    tilt_matrices(p.tilt_deg, &T, &Tinv);
    const int nb = grid_for(N, kGroundBlock, 2048);
    hipLaunchKernelGGL(k_transform_mat, dim3(ceil_div((long long)n, kBlock)), dim3(kBlock), 0, st, g.in.p, N, T, g.tilted.p);
    hipLaunchKernelGGL(k_ground_clip_flags, dim3(nb), dim3(kGroundBlock), 0, st, g.tilted.p, N, (float)(p.sensor_height + p.height_clip_range),
                       (float)(p.sensor_height - p.height_clip_range), g.flags.p);
    TRY(enqueue_compact4(c, g.tilted.p, g.flags.p, g.idx.p, N, g.clip.p, &g.d_hdr.p->pad[1], g.d_hdr.p));
    hipLaunchKernelGGL(k_ground_origin, dim3(nb), dim3(kGroundBlock), 0, st, g.flags.p, g.idx.p, (const int*)nullptr, N, g.clip_org.p);
    HIPCHK(c, hipGetLastError());
    const char* scan_timeout = "ground: compaction scan: look-back timed out";
    TRY(compact4_count(c, g.d_hdr.p, &g.h_words[0], scan_timeout));
    const int m = g.h_words[1];
    r.n_clipped = m;
    g.n_clip = m;
    if (m == 0) return leave();
    // ---- c. normal filter (:72-101) over the clipped cloud's own neighbour index
    const int nbm = grid_for(m, kGroundBlock, 2048);
    const int k = std::min(p.normal_k, m);
    const int nbq = grid_for(m, kGroundTeams, kGroundNormalMaxBlocks);
    const double cos_thr = std::cos(p.normal_filter_thresh * M_PI / 180.0);
    if (p.use_normal_filtering) {
        TRY(enqueue_nn_index(c, main_lane(c), g.clip.p, m, 1, kGroundCell, g.ix, true));
        auto* kern = p.normal_k <= 10 ? k_ground_normals<10> : k_ground_normals<20>;
        hipLaunchKernelGGL(kern, dim3(nbq), dim3(kGroundBlock), 0, st, g.clip.p, m, k, p.normal_k, (float)p.sensor_height, cos_thr, g.ix.hdr.p,
                           g.ix.blk.p, g.ix.off.p, g.ix.pts.p, g.ix.idx.p, g.normal4.p, g.flags.p, g.nbr.p);
    } else {
        HIPCHK(c, hipMemsetAsync(&g.ix.hdr.p->pad[0], 0, sizeof(int), st));
        HIPCHK(c, hipMemsetAsync(g.nbr.p, 0xff, (size_t)m * p.normal_k * sizeof(int), st));
        hipLaunchKernelGGL(k_ground_normals<10>, dim3(nbm), dim3(kGroundBlock), 0, st, g.clip.p, m, k, p.normal_k, (float)p.sensor_height, cos_thr,
                           (const GridHeader*)nullptr, (const int*)nullptr, (const int*)nullptr, (const float4*)nullptr,
                           (const int*)nullptr, g.normal4.p, g.flags.p, g.nbr.p);
    }
    // ---- the scan's state; the second compaction writes its count into it
    const size_t n_inject = g.inject.size() / 4;
    const size_t want_hyp = std::max((size_t)p.ransac_max_iterations + 1, n_inject);
    const size_t hyp_cap = (want_hyp + kGroundBatch - 1) / kGroundBatch * kGroundBatch + kGroundBatch;
    TRY(ensure(c, g.tri, hyp_cap)); TRY(ensure(c, g.coef, hyp_cap)); TRY(ensure(c, g.stat, hyp_cap)); TRY(ensure(c, g.cnt, hyp_cap));
    g.hyp_cap = hyp_cap;
    TRY(ground_table(c, first_table_words()));
    GroundState* s0 = &g.h_state[1];
    std::memset(s0, 0, sizeof(GroundState));
    s0->floor_pts = p.floor_pts_thresh;
    s0->max_it = p.ransac_max_iterations;
    s0->max_skip = p.ransac_max_iterations * 10;
    s0->inject = n_inject ? 1 : 0;
    s0->literal = p.literal_no_ground ? 1 : 0;
    s0->stream_words = (int)g.table_words;
    s0->hash_mask = (int)(2 * g.table_words - 1);
    s0->n_input = N;
    s0->thr = p.ransac_threshold;
    s0->log_prob = std::log(1.0 - p.ransac_probability);
    s0->cos_floor = std::cos(p.floor_normal_thresh * M_PI / 180.0);
    for (int a = 0; a < 3; ++a) s0->ref[a] = Tinv.m[8 + a];  // (T^-1 UnitZ).head3: the third column
    s0->s[0] = 0; s0->s[1] = 1; s0->s[2] = 2;
    s0->best_cnt = -INT_MAX;
    s0->best_h = -1;
    s0->k = 1.0;
    s0->winner[0] = s0->winner[1] = s0->winner[2] = -1;
    HIPCHK(c, hipMemcpyAsync(g.d_state.p, s0, sizeof(GroundState), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(g.nrm_t.p, 0, (size_t)m * sizeof(float4), st));  // what lies past the kept count is moved back too
    TRY(enqueue_compact4(c, g.clip.p, g.flags.p, g.idx.p, m, g.nrm_t.p, &g.d_state.p->n_normal, g.d_hdr.p));
    hipLaunchKernelGGL(k_ground_origin, dim3(nbm), dim3(kGroundBlock), 0, st, g.flags.p, g.idx.p, g.clip_org.p, m, g.nrm_org.p);
    // the cloud after the filters moved back by T^-1 (:121): /normal_ground_points, and what RANSAC runs over
    hipLaunchKernelGGL(k_transform_mat, dim3(ceil_div((long long)m, kBlock)), dim3(kBlock), 0, st, g.nrm_t.p, m, Tinv, g.nrm.p);
    HIPCHK(c, hipMemsetAsync(g.mark.p, 0, n * sizeof(int), st));
    HIPCHK(c, hipMemsetAsync(g.gflag.p, 0, (size_t)m * sizeof(int), st));
    HIPCHK(c, hipGetLastError());
    // ---- d-f. the gates and RANSAC (:143-177), on the device
    TRY(ground_ransac(c, m));
    while (g.h_state[0].overrun) {
        // the sampler ran past the table: the host continues the stream (twice the words) and the scan's loop runs again
        const size_t worst = (size_t)3 * kGroundSampleChecks * ((size_t)p.ransac_max_iterations + 1);
        if (g.table_words >= worst) return fail(c, NDT_EDEVICE, "ground: the sampler ran past the longest generator stream a scan can draw");
        r.stream_fallbacks += 1;
        TRY(ground_table(c, 2 * g.table_words));
        s0->n_normal = g.h_state[0].n_normal;
        s0->stream_words = (int)g.table_words;
        s0->hash_mask = (int)(2 * g.table_words - 1);
        HIPCHK(c, hipMemcpyAsync(g.d_state.p, s0, sizeof(GroundState), hipMemcpyHostToDevice, st));
        TRY(ground_ransac(c, m));
    }
    if (g.h_words[2]) {  // the second compaction's scan, whose flag came back with the state
        (void)hipMemsetAsync(&g.d_hdr.p->pad[0], 0, sizeof(int), st);
        return fail(c, NDT_EDEVICE, scan_timeout);
    }
    if (g.h_words[3]) return fail(c, NDT_EDEVICE, "ground: neighbour index sort: radix look-back timed out");
    const GroundState& s = g.h_state[0];
    r.found = s.found;
    r.reason = s.reason;
    for (int a = 0; a < 4; ++a) r.coeffs[a] = s.coeffs[a];
    r.n_normal = s.n_normal;
    r.n_inliers = s.n_inliers;
    r.iterations = s.iterations;
    r.skipped = s.skipped;
    for (int a = 0; a < 3; ++a) r.winner[a] = s.winner[a];
    r.k = s.k;
    return leave();
}

// One cloud of the last detect in g.cloud / g.cloud_ds; *src and *count name it
ndt_status ground_cloud_dev(ndt_ctx* c, int which, const float4** src, size_t* count) {
    GroundRun& g = c->ground;
    if (!g.valid) return fail(c, NDT_EINVAL, "no ground detect on this ctx yet");
    if (which < NDT_GROUND_CLOUD_NORMAL || which > NDT_GROUND_CLOUD_NO_GROUND) return fail(c, NDT_EINVAL, "bad ground cloud kind");
    hipStream_t st = c->stream.get();
    const ndt_ground_result& r = g.res;
    *src = nullptr;
    *count = 0;
    if (which == NDT_GROUND_CLOUD_NORMAL) {
        *src = g.nrm.p;
        *count = (size_t)r.n_normal;
    } else if (r.found) {
        const bool gr = which == NDT_GROUND_CLOUD_GROUND;
        const int n = gr ? r.n_normal : r.n_input;
        const int nb = grid_for(n, kGroundBlock, 2048);
        if (!gr) hipLaunchKernelGGL(k_ground_unmarked, dim3(nb), dim3(kGroundBlock), 0, st, g.mark.p, n, g.flags.p);
        const int* flags = gr ? g.gflag.p : g.flags.p;
        TRY(enqueue_compact4(c, gr ? g.nrm.p : g.in.p, flags, g.idx.p, n, g.cloud.p, &g.d_hdr.p->pad[1], g.d_hdr.p));
        TRY(compact4_count(c, g.d_hdr.p, &g.h_words[0], "ground: cloud compaction scan: look-back timed out"));
        *src = g.cloud.p;
        *count = (size_t)g.h_words[1];
    }
    if (*count && g.prm.cloud_leaf > 0.f) {  // downSizeNoGroundFrames (:133-134, 184-185, 205-206)
        TRY(ensure(c, g.cloud_ds, *count));
        size_t nds = 0;
        const ndt_status rs = voxel_downsample_dev(c, *src, *count, g.prm.cloud_leaf, g.cloud_ds.p, &nds);
        *src = g.cloud_ds.p;
        *count = nds;
        return rs;
    }
    return NDT_OK;
}

// ndt_ground_cloud / ndt_ground_cloud_device: up to cap points of that cloud to out4, host or device memory by the copy's
// kind; synchronises
ndt_status ground_cloud_out(ndt_ctx* c, int which, float* out4, size_t cap, size_t* n_out, hipMemcpyKind kind) {
    if (!c || !n_out || (cap && !out4)) return fail(c, NDT_EINVAL, "bad ground cloud args");
    TRY(set_dev(c));
    const float4* src = nullptr;
    const ndt_status rs = ground_cloud_dev(c, which, &src, n_out);
    if (rs != NDT_OK && rs != NDT_EOVERFLOW) return rs;
    const size_t k = std::min(cap, *n_out);
    if (k) HIPCHK(c, hipMemcpyAsync(out4, src, k * sizeof(float4), kind, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    return rs;
}

}  // namespace

extern "C" {

// filter_node.h:62-71, filter_node.cpp:36, 81, 151 and pcl::SampleConsensus's constructor
ndt_status ndt_ground_default_params(ndt_ground_params* out) {
    if (!out || out->struct_size != sizeof(ndt_ground_params)) return NDT_EINVAL;
    out->tilt_deg = 0.0;
    out->sensor_height = 2.0;
    out->height_clip_range = 2.5;
    out->floor_pts_thresh = 512;
    out->floor_normal_thresh = 10.0;
    out->use_normal_filtering = 1;
    out->normal_filter_thresh = 20.0;
    out->normal_k = 10;
    out->ransac_threshold = 0.1;
    out->ransac_probability = 0.99;
    out->ransac_max_iterations = 1000;
    out->literal_no_ground = 0;
    out->cloud_leaf = 0.2f;
    return NDT_OK;
}

int ndt_ground_batch(void) { return kGroundBatch; }

ndt_status ndt_ground_detect_device(ndt_ctx* c, const ndt_ground_params* prm, const float* d_in4, size_t n, ndt_ground_result* result) {
    if (!c || !result || (n && !d_in4) || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad ground args");
    TRY(set_dev(c));
    return ground_detect_dev(c, prm, reinterpret_cast<const float4*>(d_in4), n, result);
}

ndt_status ndt_ground_detect(ndt_ctx* c, const ndt_ground_params* prm, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset,
                             ndt_ground_result* result) {
    if (!c || !result || (n && !xyzi) || !xyzi_layout_ok(stride_bytes, intensity_offset) || n > 0x7fffffffULL)
        return fail(c, NDT_EINVAL, "bad ground args");
    TRY(set_dev(c));
    if (n == 0) return ground_detect_dev(c, prm, nullptr, 0, result);
    const std::vector<float> tmp = pack_cloud4(xyzi, n, stride_bytes, intensity_offset);
    TRY(ensure(c, c->ground.in, n));
    HIPCHK(c, hipMemcpyAsync(c->ground.in.p, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));  // tmp goes with this scope
    return ground_detect_dev(c, prm, c->ground.in.p, n, result);
}

ndt_status ndt_ground_cloud_device(ndt_ctx* c, int which, float* d_out4, size_t cap, size_t* n_out) {
    return ground_cloud_out(c, which, d_out4, cap, n_out, hipMemcpyDeviceToDevice);
}

ndt_status ndt_ground_cloud(ndt_ctx* c, int which, float* out4, size_t cap, size_t* n_out) {
    return ground_cloud_out(c, which, out4, cap, n_out, hipMemcpyDeviceToHost);
}

ndt_status ndt_filter_ground_scan(ndt_ctx* c, const ndt_filter_params* fprm, const ndt_ground_params* gprm, const float* d_in4, size_t n,
                                  float* d_out4, size_t* n_out, ndt_ground_result* result) {
    if (!c || !result) return fail(c, NDT_EINVAL, "bad ground args");
    TRY(ndt_filter_scan_device(c, fprm, d_in4, n, d_out4, n_out));
    return ground_detect_dev(c, gprm, reinterpret_cast<const float4*>(d_out4), *n_out, result);
}

ndt_status ndt_ground_last_normals(ndt_ctx* c, float* normal4, int* keep, int* origin, int* nbr, size_t cap, size_t* n_out) {
    if (!c || !n_out) return fail(c, NDT_EINVAL, "null argument");
    GroundRun& g = c->ground;
    if (!g.valid) return fail(c, NDT_EINVAL, "no ground detect on this ctx yet");
    TRY(set_dev(c));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    *n_out = (size_t)g.n_clip;
    const size_t k = std::min(cap, (size_t)g.n_clip);
    if (!k) return NDT_OK;
    if (normal4) HIPCHK(c, hipMemcpy(normal4, g.normal4.p, k * sizeof(float4), hipMemcpyDeviceToHost));
    if (origin) HIPCHK(c, hipMemcpy(origin, g.clip_org.p, k * sizeof(int), hipMemcpyDeviceToHost));
    if (nbr) HIPCHK(c, hipMemcpy(nbr, g.nbr.p, k * (size_t)g.prm.normal_k * sizeof(int), hipMemcpyDeviceToHost));
    if (keep) {
        // the filter's flags were the second compaction's input; a cloud request may have reused the buffer since, so the
        // flag is read off the kept points' indices: origin of the kept cloud -> position in the clipped cloud
        std::vector<int> org(g.n_clip), kept((size_t)g.res.n_normal);
        HIPCHK(c, hipMemcpy(org.data(), g.clip_org.p, (size_t)g.n_clip * sizeof(int), hipMemcpyDeviceToHost));
        if (!kept.empty()) HIPCHK(c, hipMemcpy(kept.data(), g.nrm_org.p, kept.size() * sizeof(int), hipMemcpyDeviceToHost));
        size_t at = 0;  // both lists ascend
        for (size_t i = 0; i < (size_t)g.n_clip; ++i) {
            const bool on = at < kept.size() && kept[at] == org[i];
            if (on) ++at;
            if (i < k) keep[i] = on ? 1 : 0;
        }
    }
    return NDT_OK;
}

ndt_status ndt_ground_last_hypotheses(ndt_ctx* c, int* triples, float* coeffs, int* counts, int* status, size_t cap, size_t* n_out) {
    if (!c || !n_out) return fail(c, NDT_EINVAL, "null argument");
    GroundRun& g = c->ground;
    if (!g.valid) return fail(c, NDT_EINVAL, "no ground detect on this ctx yet");
    TRY(set_dev(c));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    const size_t seen = g.res.n_normal > 0 && g.h_state ? (size_t)g.h_state[0].seen : 0;
    *n_out = g.n_clip > 0 ? seen : 0;
    const size_t k = std::min(cap, *n_out);
    if (!k) return NDT_OK;
    if (triples) {
        std::vector<int4> t(k);
        HIPCHK(c, hipMemcpy(t.data(), g.tri.p, k * sizeof(int4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < k; ++i) { triples[3 * i] = t[i].x; triples[3 * i + 1] = t[i].y; triples[3 * i + 2] = t[i].z; }
    }
    if (coeffs) HIPCHK(c, hipMemcpy(coeffs, g.coef.p, k * sizeof(float4), hipMemcpyDeviceToHost));
    if (counts) HIPCHK(c, hipMemcpy(counts, g.cnt.p, k * sizeof(int), hipMemcpyDeviceToHost));
    if (status) HIPCHK(c, hipMemcpy(status, g.stat.p, k * sizeof(int), hipMemcpyDeviceToHost));
    return NDT_OK;
}

ndt_status ndt_ground_set_samples(ndt_ctx* c, const int* triples, size_t n_triples) {
    if (!c || (n_triples && !triples) || n_triples > (1u << 20)) return fail(c, NDT_EINVAL, "bad ground samples");
    std::vector<int>& v = c->ground.inject;  // as int4 (i0, i1, i2, status), the layout of the hypotheses' buffer
    v.assign(4 * n_triples, GROUND_SAMPLE_OK);
    for (size_t i = 0; i < n_triples; ++i)
        for (int a = 0; a < 3; ++a) v[4 * i + a] = triples[3 * i + a];
    return NDT_OK;
}

}  // extern "C"
