// host_target.hip — the target side of the registration: setInputTarget's device voxel build, the merge-extended
// build, the re-run of a flagged build, and the grid's inspection entry points.
#include "ndt_host.h"

namespace ndt::host {

namespace {

// dense grid: grown lazily to twice the largest cell count seen (capped at 1 Gi cells = 4 GiB)
ndt_status grow_grid(ndt_ctx* c) {
    const long long want_cells = std::min<long long>(std::max<long long>(2 * c->grid_cells_seen, 16ll << 20), 1ll << 30);
    if ((long long)c->grid.cap < want_cells) TRY(ensure(c, c->grid, (size_t)want_cells));
    return NDT_OK;
}

ndt_status alloc_cloud_buffers(ndt_ctx* c, size_t max_cloud) {
    TRY(ensure(c, c->recs, max_cloud)); TRY(ensure(c, c->cent, max_cloud)); TRY(ensure(c, c->icovd, max_cloud * 9));
    TRY(ensure(c, c->evals, max_cloud * 3)); TRY(ensure(c, c->cloud_key, max_cloud));
    return NDT_OK;
}

constexpr int kFinalize3WavesMaxPoints = 4 << 20;

// Target buffers for M points: records, lookup structure, cloud spans; returns the finalize's workgroup count.
ndt_status prepare_target_buffers(ndt_ctx* c, int M, int* nb_cloud) {
    TRY(grow_grid(c));
    const size_t max_cloud = std::max(1, M / std::max(1, c->prm.min_points_per_voxel) + 1);
    TRY(alloc_cloud_buffers(c, max_cloud));
    unsigned l = 6;
    while (l < 30 && (1ull << l) < 4ull * max_cloud) ++l;
    c->max_log2cap = l;
    TRY(ensure(c, c->table, (size_t)1 << l));
    *nb_cloud = std::max(1, ceil_div((long long)max_cloud, kBlock));
    TRY(ensure(c, c->s.cloud_span, (size_t)*nb_cloud * kBlock));  // every finalize thread loads its entry
    TRY(ensure(c, c->valid_part, max_cloud / 64 + 1));
    return NDT_OK;
}

// one thread per cloud voxel: moments, eigen inflation, inverse, and its lookup entry
ndt_status launch_finalize(ndt_ctx* c, int M, int nb_cloud) {
    // three waves per SIMD below ~4 M target points (C2 / C3 localmaps), two above (C5: the larger register file wins)
    auto* fin = M < kFinalize3WavesMaxPoints ? k_leaf_finalize<3> : k_leaf_finalize<2>;
    hipLaunchKernelGGL(fin, dim3(nb_cloud), dim3(kBlock), 0, c->stream.get(), c->target_ptr, c->s.k0.p, c->s.k1.p, c->s.v0.p,
                       c->s.v1.p, c->s.cloud_span.p, c->d_hdr.p, c->recs.p, c->cent.p, c->icovd.p, c->cloud_key.p,
                       c->evals.p, c->grid.p, c->table.p, c->valid_part.p);
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

ndt_status enqueue_target_build(ndt_ctx* c) {
    c->inc_ok = false;
    ++c->n_builds_full;
    const int M = c->M;
    int nb_cloud = 0;
    TRY(prepare_target_buffers(c, M, &nb_cloud));
    // precision_mode 2 (ndt_cpu) bins like cpu::VoxelGrid (division), the others like pclomp's VGC (multiplication)
    // keys, sort, segments and the cloud voxels (>= min points) in key order; then the lookup structure chosen and
    // cleared, then the finalize
    TRY(enqueue_bin_and_sort(c, main_lane(c), c->target_ptr, M, c->target_dense, c->d_hdr.p, c->prm.resolution, 0, c->prm.precision_mode == 2 ? 1 : 0,
                             c->s.cloud_span.p, radix_launch_passes(c)));
    TRY(launch_finalize(c, M, nb_cloud));
    // a pclomp grid over a dense cloud can be extended by merge (its sorted keys / indices stay in c->s)
    c->inc_ok = c->prm.precision_mode != 2 && c->target_dense == 1 && M > 0;
    return NDT_OK;
}

// The target grown by n_new points appended after its n_old (k_merge_append): the new points' min/max (the current
// header saved and its box folded in), their keys in the grown box and their radix sort (own scratch), the merge with
// the current sort, then the same segment scan, cloud scan and finalize as a full build.  Bitwise the grid of
// enqueue_target_build over the n_old + n_new points.
ndt_status enqueue_target_append(ndt_ctx* c, int n_old, int n_new, const float4* new_src) {
    const int M = n_old + n_new;
    int nb_cloud = 0;
    TRY(prepare_target_buffers(c, M, &nb_cloud));
    Lane Q{c->stream.get(), c->s_inc};
    // new_src: the new points are read there and stored after the old ones by k_minmax (no separate copy launch)
    float4* copy_to = new_src ? const_cast<float4*>(c->target_ptr) + n_old : nullptr;
    const float4* pts_new = new_src ? new_src : c->target_ptr + n_old;
    const int nq = std::max(n_new, 1);
    const int nb_mm = grid_for(nq, 4 * kBlock, 1024);
    TRY(ensure(c, Q.s.mm, (size_t)nb_mm * 7));
    const int items = radix_items(c, nq);
    const int nb_sort = std::max(1, ceil_div(nq, kBlock * items));
    TRY(ensure(c, Q.s.k0, nq)); TRY(ensure(c, Q.s.v0, nq)); TRY(ensure(c, Q.s.k1, nq)); TRY(ensure(c, Q.s.v1, nq));
    TRY(ensure(c, Q.s.radix_aux, kRadixAuxWords));
    TRY(ensure(c, Q.s.radix_status, radix_status_words(nb_sort)));
    TRY(ensure(c, c->s.seg_start, (size_t)M + 1));
    hipLaunchKernelGGL(k_minmax, dim3(nb_mm), dim3(kBlock), 0, c->stream.get(), pts_new, n_new, 1, Q.s.mm.p, Q.s.radix_aux.p, c->d_clk.p + 3,
                       c->d_hdr.p, c->d_hdr_prev.p, copy_to);
    // the target's points are all in place now: getFitnessScore's index (fit lane) may start beside the rest
    if (c->tgt_ev_valid) HIPCHK(c, hipEventRecord(c->ev_tgt.get(), c->stream.get()));
    // k_keys also clears the grown target's lookup structure (its whole dense grid or hash table): sized for that as well
    // as for the new points, capped as in a full build
    const long long clear_words = std::max<long long>((long long)c->grid.cap, 2LL << c->max_log2cap) / 4;
    const int nb_keys = std::max(1, (int)std::min<long long>(std::max<long long>(ceil_div(nq, 4 * kBlock), ceil_div(clear_words, 4LL * kBlock)), 512));
    hipLaunchKernelGGL(k_keys, dim3(nb_keys), dim3(kBlock), 0, c->stream.get(), pts_new, n_new, 1, Q.s.mm.p, nb_mm, c->d_hdr.p, c->prm.resolution,
                       c->prm.min_points_per_voxel, c->prm.min_covar_eigvalue_mult, 0, 0, Q.s.k0.p, Q.s.v0.p, Q.s.radix_aux.p,
                       Q.s.radix_status.p, (int)radix_status_words(nb_sort), c->grid.p, (long long)c->grid.cap, c->table.p, 1LL << c->max_log2cap,
                       c->d_hdr_prev.p, n_old);
    const int passes = radix_launch_passes(c);
    for (int pass = 0; pass < passes; ++pass)
        launch_radix_pass(c, Q, items, nb_sort, Q.s.k0.p, Q.s.v0.p, Q.s.k1.p, Q.s.v1.p, n_new, pass, c->d_hdr.p, c->d_hdr.p, passes - 1);
    hipLaunchKernelGGL(k_merge_append, dim3(std::max(1, ceil_div(M, kMergeTileKeys))), dim3(kBlock), 0, c->stream.get(), c->s.k0.p, c->s.v0.p,
                       c->s.k1.p, c->s.v1.p, c->d_hdr_prev.p, n_old, Q.s.k0.p, Q.s.v0.p, Q.s.k1.p, Q.s.v1.p, n_new, c->d_hdr.p,
                       c->target_ptr);
    const Lane L = main_lane(c);
    const int nb_seg = std::max(1, ceil_div(M, kTileKeys));
    ScanCtx sc, sc2;
    TRY(scan_ctx(c, L, nb_seg, &sc));
    hipLaunchKernelGGL(k_seg_scan, dim3(nb_seg), dim3(kBlock), 0, c->stream.get(), c->s.k0.p, c->s.k1.p, M, c->d_hdr.p, c->s.seg_start.p, sc);
    TRY(scan_ctx(c, L, nb_seg, &sc2));
    hipLaunchKernelGGL(k_cloud_scan, dim3(nb_seg), dim3(kBlock), 0, c->stream.get(), c->s.seg_start.p, M, c->d_hdr.p, c->s.cloud_span.p, sc2,
                       c->max_log2cap);
    TRY(launch_finalize(c, M, nb_cloud));
    return NDT_OK;
}

}  // namespace

// No stream events around the build unless getFitnessScore's index uses them: an event recorded between two kernels leaves
// the stream idle ~6 us (rocprofv3, C2 step).  The build's time comes from device stamps (k_minmax's start .. the align's
// k_align_init, read back with the align), the largest grid seen from the align state (grid_cells).
ndt_status build_target(ndt_ctx* c) {
    ++c->tgt_gen;
    // the target's points are in place: getFitnessScore's index (fit lane) may start beside the build
    c->tgt_ev_valid = c->lanes.fit_tgt_used;
    if (c->tgt_ev_valid) HIPCHK(c, hipEventRecord(c->ev_tgt.get(), c->stream.get()));
    TRY(enqueue_target_build(c));
    c->build_unchecked = true;
    c->built_since_align = true;
    c->grid_valid = true;
    c->fit_valid = false;
    c->grid_res = c->prm.resolution;
    c->have_result = false;
    return NDT_OK;
}

// A target build whose sort flagged an error (GridHeader::pad[0]) is queued again from scratch: all four radix passes,
// tiles by atomic ticket from now on if a look-back timed out (the blockIdx.x tile order relies on each XCD dispatching
// its workgroups in increasing order, observed but not guaranteed when other streams' kernels hold the CUs; a ticket
// tile waits only on tiles that started before it), a fresh sort where a merge could not be exact.  Same grid as a
// first build that had not failed.
ndt_status rerun_build(ndt_ctx* c, int berr) {
    ++c->n_builds_rerun;
    if (berr & kBuildErrLookback) {
        c->opt.tile_tickets = true;
        ++c->n_rerun_lookback;
    }
    c->inc_ok = false;
    c->rerun_full = true;
    const ndt_status st = build_target(c);
    c->rerun_full = false;
    return st;
}

// The synchronous readers of the target grid other than an align (grid inspection, single passes, calculateScore): the
// error bits of a build no align has checked yet, read back now; a flagged build is re-run.
ndt_status settle_build(ndt_ctx* c) {
    if (!c->build_unchecked || !c->grid_valid) return NDT_OK;
    for (int attempt = 0;; ++attempt) {
        HIPCHK(c, hipMemcpyAsync(c->h_hdr.get(), c->d_hdr.p, sizeof(GridHeader), hipMemcpyDeviceToHost, c->stream.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
        const int berr = c->h_hdr->pad[0];
        if (!berr) break;
        if (attempt > 0) return fail(c, NDT_EDEVICE, "target build failed twice (error bits " + std::to_string(berr) + ")");
        TRY(rerun_build(c, berr));
    }
    c->build_unchecked = false;
    note_grid_width(c, c->h_hdr->cells, c->target_dense);
    return NDT_OK;
}

ndt_status upload_points(ndt_ctx* c, DevBuf<float4>& dst, const float* xyz, size_t n, size_t stride_bytes) {
    TRY(ensure(c, dst, n));
    const std::vector<float> tmp = pack_cloud4(xyz, n, stride_bytes, -1);
    if (n) HIPCHK(c, hipMemcpyAsync(dst.p, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    return NDT_OK;
}

// cpu::NormalDistributionsTransform::updateVoxelGrid (ndt_cpu/NormalDistributionsTransform.h:39, driven at
// odom_node.cpp:344-345 when incremental voxel update is on): the new points join the target after the old ones.  The
// cpu::VoxelGrid keeps per-voxel sums that the new points extend in input order, so every voxel's statistics equal those
// of a grid built over old + new points in that order; the device appends the points to its owned target copy and
// rebuilds the grid (one sort of the whole target, ~0.2 ms for 2 M points).  Known difference: ndt_cpu's incremental
// path leaves a voxel that was rejected (points_per_voxel = -1) and then receives points with a count of -1 + k, which
// hides it from radiusSearch; the rebuild counts it afresh.
static ndt_status append_target(ndt_ctx* c, const float4* d_new, const float* h_new, size_t n, size_t stride_bytes) {
    TRY(set_dev(c));
    TRY(main_after_fit(c, false));  // the fit lane may still read the owned copy
    if (n == 0) return NDT_OK;
    const size_t m0 = c->has_target ? (size_t)c->M : 0, m = m0 + n;
    if (m > 0x7fffffffULL) return fail(c, NDT_EINVAL, "target too large");
    if (c->target_ptr != c->target.p || c->target.cap < m) {
        // a larger owned buffer (or the first owned copy of a caller-referenced target), old points first
        DevBuf<float4> nb;
        TRY(ensure(c, nb, std::max(m, m0 + m0 / 2)));
        if (m0) HIPCHK(c, hipMemcpyAsync(nb.p, c->target_ptr, m0 * sizeof(float4), hipMemcpyDeviceToDevice, c->stream.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
        std::swap(c->target.p, nb.p);  // nb frees the previous copy
        std::swap(c->target.cap, nb.cap);
    }
    if (d_new) {
        HIPCHK(c, hipMemcpyAsync(c->target.p + m0, d_new, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream.get()));
    } else {
        const std::vector<float> tmp = pack_cloud4(h_new, n, stride_bytes, -1);
        HIPCHK(c, hipMemcpyAsync(c->target.p + m0, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    }
    c->target_ptr = c->target.p;
    c->M = (int)m;
    if (!c->has_target) c->target_dense = 1;
    c->has_target = true;
    return build_target(c);
}

}  // namespace ndt::host

extern "C" {

ndt_status ndt_set_target(ndt_ctx* c, const float* xyz, size_t n, size_t stride_bytes, int is_dense) {
    if (!c || (n && !xyz) || stride_bytes < 12 || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad target");
    TRY(set_dev(c));
    TRY(main_after_fit(c, false));  // the fit lane may still read the owned copy
    TRY(upload_points(c, c->target, xyz, n, stride_bytes));
    c->target_ptr = c->target.p;
    c->M = (int)n;
    c->target_dense = is_dense ? 1 : 0;
    c->has_target = true;
    return build_target(c);
}

ndt_status ndt_set_target_device(ndt_ctx* c, const float* d_xyz4, size_t n, int is_dense) {
    if (!c || (n && !d_xyz4) || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad target");
    TRY(set_dev(c));
    // like pcl::Registration::setInputTarget the cloud is referenced, not copied: the caller keeps the
    // device buffer alive and unmodified while this ctx uses it (until the next set_target)
    c->target_ptr = reinterpret_cast<const float4*>(d_xyz4);
    c->M = (int)n;
    c->target_dense = is_dense ? 1 : 0;
    c->has_target = true;
    return build_target(c);
}

// setInputTarget of a cloud that extends the current target: its first n_old points are the current target's (same
// values, same order) and n_new follow (odom_node.cpp:233 / 349 between localmap resets: pc_target_ is the localmap,
// which only grows by appends).  The grid is the one ndt_set_target_device builds; when the current sort can be reused
// it is built by merging the new points' sort into it (enqueue_target_append), otherwise from scratch.
ndt_status ndt_set_target_append_device(ndt_ctx* c, float* d_xyz4, size_t n_old, size_t n_new, int is_dense,
                                        const float* d_new4) {
    if (!c || ((n_old + n_new) && !d_xyz4) || n_old + n_new > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad target");
    TRY(set_dev(c));
    const float4* new_src = reinterpret_cast<const float4*>(d_new4);
    if (new_src == reinterpret_cast<const float4*>(d_xyz4) + n_old) new_src = nullptr;  // already in place
    const size_t m = n_old + n_new;
    const bool disabled = std::getenv("NDT_NO_TARGET_MERGE") != nullptr;  // A/B runs and tests
    const bool merge = !disabled && c->inc_ok && c->has_target && c->grid_valid && is_dense && c->target_dense == 1 &&
                       (size_t)c->M == n_old && n_old > 0 && c->grid_res == c->prm.resolution && c->prm.precision_mode != 2 &&
                       c->s.k0.cap >= m && c->s.v0.cap >= m && c->s.k1.cap >= m && c->s.v1.cap >= m;
    c->target_ptr = reinterpret_cast<const float4*>(d_xyz4);
    c->M = (int)m;
    c->target_dense = is_dense ? 1 : 0;
    c->has_target = true;
    if (!merge) {
        if (new_src && n_new)
            TRY(ndt_memcpy_d2d(c, d_xyz4 + 4 * n_old, d_new4, n_new * sizeof(float4)));
        return build_target(c);
    }
    ++c->tgt_gen;
    c->tgt_ev_valid = c->lanes.fit_tgt_used;
    if (c->tgt_ev_valid && !new_src) HIPCHK(c, hipEventRecord(c->ev_tgt.get(), c->stream.get()));
    const ndt_status st = enqueue_target_append(c, (int)n_old, (int)n_new, new_src);
    if (st != NDT_OK) {
        c->inc_ok = false;
        return st;
    }
    ++c->n_builds_merge;
    c->build_unchecked = true;
    c->built_since_align = true;
    c->grid_valid = true;
    c->fit_valid = false;
    c->grid_res = c->prm.resolution;
    c->have_result = false;
    return NDT_OK;
}

ndt_status ndt_update_target(ndt_ctx* c, const float* xyz, size_t n, size_t stride_bytes) {
    if (!c || (n && !xyz) || stride_bytes < 12 || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad target update");
    return append_target(c, nullptr, xyz, n, stride_bytes);
}

ndt_status ndt_update_target_device(ndt_ctx* c, const float* d_xyz4, size_t n) {
    if (!c || (n && !d_xyz4) || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad target update");
    return append_target(c, reinterpret_cast<const float4*>(d_xyz4), nullptr, n, 16);
}

ndt_status ndt_grid_info(ndt_ctx* c, int header[16]) {
    if (!c || !header) return fail(c, NDT_EINVAL, "null argument");
    if (!c->has_target) return fail(c, NDT_ENOTARGET, "no input target");
    TRY(set_dev(c));
    if (!c->grid_valid) TRY(build_target(c));
    TRY(settle_build(c));
    HIPCHK(c, hipMemcpyAsync(c->h_hdr.get(), c->d_hdr.p, sizeof(GridHeader), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    const GridHeader& h = *c->h_hdr;
    c->grid_cells_seen = std::max(c->grid_cells_seen, h.cells);
    for (int a = 0; a < 3; ++a) { header[a] = h.min_b[a]; header[3 + a] = h.max_b[a]; header[6 + a] = h.div_b[a]; header[9 + a] = h.divb_mul[a]; }
    header[12] = h.n_leaves;
    header[13] = h.n_cloud;
    header[14] = h.overflow;
    // usable voxels: the finalize's per-wave counts
    long long nv = 0;
    if (h.n_cloud > 0 && !h.empty) {
        std::vector<int> part((size_t)(h.n_cloud + 63) / 64);
        HIPCHK(c, hipMemcpy(part.data(), c->valid_part.p, part.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int v : part) nv += v;
    }
    header[15] = (int)nv;
    return NDT_OK;
}

ndt_status ndt_grid_leaves(ndt_ctx* c, int* keys, int* npts, double* mean, double* icov9, float* centroid3, int cap, int* n_out) {
    int hdr[16];
    TRY(ndt_grid_info(c, hdr));
    const int n = std::min(hdr[13], std::max(cap, 0));
    *n_out = hdr[13];
    if (n == 0) return NDT_OK;
    std::vector<VoxelRec> r(n);
    std::vector<float4> ce(n);
    std::vector<int> k(n);
    std::vector<double> ic((size_t)n * 9);
    HIPCHK(c, hipMemcpy(r.data(), c->recs.p, n * sizeof(VoxelRec), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ce.data(), c->cent.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(k.data(), c->cloud_key.p, n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ic.data(), c->icovd.p, (size_t)n * 9 * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        if (keys) keys[i] = k[i];
        if (npts) npts[i] = r[i].npts;
        if (mean) for (int a = 0; a < 3; ++a) mean[3 * i + a] = r[i].mean[a];
        if (icov9) for (int a = 0; a < 9; ++a) icov9[9 * i + a] = ic[(size_t)9 * i + a];
        if (centroid3) { centroid3[3 * i] = ce[i].x; centroid3[3 * i + 1] = ce[i].y; centroid3[3 * i + 2] = ce[i].z; }
    }
    return NDT_OK;
}

}  // extern "C"
