// host_lanes.hip — the two side lanes (getFitnessScore, keyframe insertion) and their host threads, the
// nearest-neighbour index, and the error text of a call (the caller's, or a lane thread's own).
#include "ndt_host.h"

namespace ndt::host {

// On a side lane's host thread: where fail() puts the error text (the ctx's error string belongs to the caller's thread)
static thread_local std::string* tl_err = nullptr;

ndt_status fail(ndt_ctx* c, ndt_status st, const std::string& msg) {
    if (tl_err) *tl_err = msg;  // a side lane's host thread: reported by the lane's result call
    else if (c) c->err = msg;
    return st;
}

void LaneWorker::run() {
    (void)hipSetDevice(device);
    std::string local;
    tl_err = &local;
    for (;;) {
        std::function<ndt_status()> f;
        bool skip;
        {
            std::unique_lock<std::mutex> g(mu);
            cv_job.wait(g, [this] { return stop || !jobs.empty(); });
            if (jobs.empty()) return;  // stopped, nothing left
            f = std::move(jobs.front());
            jobs.pop_front();
            // after a failure the jobs queued behind it are dropped until take_error: they would launch on buffers the
            // failed job left unbuilt (e.g. a getFitnessScore query on an index whose allocation failed)
            skip = st != NDT_OK;
        }
        local.clear();
        ndt_status s = NDT_OK;
        if (!skip) {
            std::shared_lock<std::shared_mutex> g(*capture_mu);
            s = f();
        }
        {
            std::lock_guard<std::mutex> g(mu);
            if (s != NDT_OK && st == NDT_OK) {
                st = s;
                msg = local;
            }
            --pending;
        }
        cv_idle.notify_all();
    }
}

// the side lanes (fit_stream / ins_stream), created on the first side-lane call, at the lowest stream priority (the
// main stream, whose target build and align are the scan loop's critical path, has the highest).  Built apart and
// moved into the ctx whole: a step that fails leaves the ctx without side lanes, and the next call starts over.
static ndt_status side_lanes(ndt_ctx* c) {
    if (c->lanes.fit_worker) return NDT_OK;
    int least = 0, greatest = 0;
    HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    SideLanes L;
    TRY(make_stream(c, L.fit_stream, least));
    TRY(make_stream(c, L.ins_stream, least));
    for (Event* e : {&L.ev_main_fit, &L.ev_main_ins, &L.ev_fit_src, &L.ev_fit_tgt, &L.ev_fit, &L.ev_ins})
        TRY(make_event(c, *e, hipEventDisableTiming));
    TRY(ensure(c, L.d_hdr_ins, 1));
    L.ins_worker = std::make_unique<LaneWorker>(c->device, &c->capture_mu);
    L.fit_worker = std::make_unique<LaneWorker>(c->device, &c->capture_mu);
    c->lanes = std::move(L);
    return NDT_OK;
}

// the main stream continues after the fit-lane work that reads what it is about to rewrite: the last query that read the
// ctx's source (source = true) or the last index build that read the ctx's target points (source = false)
ndt_status main_after_fit(ndt_ctx* c, bool source) {
    if (!(source ? c->lanes.fit_src_used : c->lanes.fit_tgt_used)) return NDT_OK;
    std::string msg;
    // every queued fit-lane launch issued; a failure is reported here and cleared (it would otherwise block every later
    // target / source change), and the index it may have left unbuilt is dropped
    const ndt_status st = c->lanes.fit_worker->take_error(&msg);
    if (st != NDT_OK) {
        c->fit_valid = false;
        c->lanes.fit_pending = false;
        return fail(c, st, "getFitnessScore: " + msg);
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream.get(), source ? c->lanes.ev_fit_src.get() : c->lanes.ev_fit_tgt.get(), 0));
    return NDT_OK;
}

// nearest-neighbour index over all target points (built on the first fitness query after a target change)
// Builds an NNIndex over n device points (cell = base cell size, doubled by k_header until the block-major key range
// fits).  Uses the ctx's sort scratch; stream-ordered.
ndt_status enqueue_nn_index(ndt_ctx* c, Lane L, const float4* pts, int n, int dense, float cell, NNIndex& ix, bool want_idx) {
    TRY(enqueue_bin_and_sort(c, L, pts, n, dense, ix.hdr.p, cell, 1));
    TRY(ensure(c, ix.pts, std::max(n, 1))); TRY(ensure(c, ix.keys, std::max(n, 1))); TRY(ensure(c, ix.start, (size_t)n + 1));
    if (want_idx) TRY(ensure(c, ix.idx, std::max(n, 1)));
    const int nb = grid_for(n, kBlock, 4096);
    hipLaunchKernelGGL(k_fit_gather, dim3(nb), dim3(kBlock), 0, L.st, pts, L.s.k0.p, L.s.k1.p, L.s.v0.p, L.s.v1.p,
                       L.s.seg_start.p, n, ix.hdr.p, ix.pts.p, ix.keys.p, ix.start.p, want_idx ? ix.idx.p : nullptr);
    // occupied blocks: flags -> exclusive scan -> block table + 513 cell offsets per occupied block
    const size_t max_occ = (size_t)std::max(1, std::min(n, kFitMaxBlocks));
    TRY(ensure(c, L.s.flags, std::max(n, 1))); TRY(ensure(c, L.s.cloud_idx, std::max(n, 1)));
    TRY(ensure(c, ix.blk, (size_t)kFitMaxBlocks)); TRY(ensure(c, ix.off, max_occ * (kFitBlockCells + 1)));
    const int nb_pts = std::max(1, ceil_div(n, kBlock));
    hipLaunchKernelGGL(k_fit_block_flags, dim3(nb_pts), dim3(kBlock), 0, L.st, ix.keys.p, ix.hdr.p, L.s.flags.p);
    TRY(enqueue_scan(c, L, L.s.flags.p, std::max(n, 1), &ix.hdr.p->n_leaves, L.s.cloud_idx.p, &ix.hdr.p->n_blocks_occ, ix.hdr.p));
    hipLaunchKernelGGL(k_fit_block_clear, dim3(std::max(1, std::min(kFitMaxBlocks / kBlock, 256))), dim3(kBlock), 0, L.st,
                       ix.blk.p, ix.hdr.p);
    hipLaunchKernelGGL(k_fit_tables, dim3(nb_pts), dim3(kBlock), 0, L.st, ix.keys.p, ix.start.p, L.s.flags.p,
                       L.s.cloud_idx.p, ix.hdr.p, ix.blk.p, ix.off.p);
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

// getFitnessScore's index over the current target, queued on the fit lane behind the target's points (ev_tgt, recorded
// ahead of the voxel build, so the two builds run side by side); issued by the lane's host thread
ndt_status ensure_fit_index(ndt_ctx* c) {
    TRY(side_lanes(c));
    if (c->lanes.fit_worker->failed()) {
        // a fit-lane job failed (possibly this index's build): report it now instead of querying a half-built index
        std::string msg;
        const ndt_status st = c->lanes.fit_worker->take_error(&msg);
        c->fit_valid = false;
        c->lanes.fit_pending = false;
        return fail(c, st, "getFitnessScore: " + msg);
    }
    if (c->fit_valid) return NDT_OK;
    const float4* pts = c->target_ptr;
    const int M = c->M, dense = c->target_dense;
    const float res = c->prm.resolution;
    if (!c->tgt_ev_valid) {  // the first index of this ctx: behind everything queued so far (the build included)
        HIPCHK(c, hipEventRecord(c->ev_tgt.get(), c->stream.get()));
        c->tgt_ev_valid = true;
    }
    c->fit_ix_gen = c->tgt_gen;
    const bool want_idx = c->icp.used;
    c->lanes.fit_worker->post([c, pts, M, dense, res, want_idx]() -> ndt_status {
        HIPCHK(c, hipStreamWaitEvent(c->lanes.fit_stream.get(), c->ev_tgt.get(), 0));
        // target points binned in 8x8x8-cell blocks (block-major keys, same stable radix sort as the voxel build)
        TRY(enqueue_nn_index(c, Lane{c->lanes.fit_stream.get(), c->lanes.s_fit}, pts, M, dense, res, c->fit_ix, want_idx));
        HIPCHK(c, hipEventRecord(c->lanes.ev_fit_tgt.get(), c->lanes.fit_stream.get()));
        return NDT_OK;
    });
    c->lanes.fit_tgt_used = true;
    c->fit_valid = true;
    return NDT_OK;
}

// The target's index with the points' original indices (ICP, GICP), built and visible to the main stream; prefix names
// the caller in the error text.
ndt_status target_nn_index(ndt_ctx* c, const char* prefix) {
    if (!c->icp.used) {  // the index carries the original-index word from now on
        c->icp.used = true;
        c->fit_valid = false;  // rebuilt behind the fit lane's queued queries (FIFO)
    }
    TRY(ensure_fit_index(c));
    std::string msg;
    const ndt_status st = c->lanes.fit_worker->take_error(&msg);  // the index build has been issued
    if (st != NDT_OK) {
        c->fit_valid = false;
        c->lanes.fit_pending = false;
        return fail(c, st, std::string(prefix) + ": nearest-neighbour index: " + msg);
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream.get(), c->lanes.ev_fit_tgt.get(), 0));
    return NDT_OK;
}

// The error bits of ix's sort (GridHeader::pad[0], as k_fitness reports them through its count); a flagged target index
// is dropped.  The caller has synchronised the main stream behind the kernels that read ix, so the read is one blocking
// copy (an asynchronous copy into pageable memory and a second synchronise cost an align some 10 us more).
ndt_status check_index_sort(ndt_ctx* c, const NNIndex& ix, const char* prefix) {
    int ix_err = 0;
    HIPCHK(c, hipMemcpy(&ix_err, &ix.hdr.p->pad[0], sizeof(int), hipMemcpyDeviceToHost));
    if (ix_err) {
        if (&ix == &c->fit_ix) c->fit_valid = false;
        return fail(c, NDT_EDEVICE, std::string(prefix) + ": nearest-neighbour index sort: radix look-back timed out");
    }
    return NDT_OK;
}

// getFitnessScore of N device points src (the ctx's source, or a caller cloud that stays valid until the result call)
static ndt_status fitness_enqueue(ndt_ctx* c, const float* T, double max_range, const float4* src, int N, bool ctx_source,
                                  bool index_ready = false) {
    TRY(set_dev(c));
    if (!index_ready) TRY(ensure_fit_index(c));
    // getFitnessScore uses final_transformation_: the last align's result (identity before any align)
    Mat4f Tm;
    for (int k = 0; k < 16; ++k) Tm.m[k] = T ? T[k] : (c->have_result ? last_final(c)[k] : (k % 5 == 0 ? 1.f : 0.f));
    // the query runs on the fit lane behind the main stream's work so far (the source copy, the align whose transform
    // it applies: the marker is recorded here, on the caller's thread) and beside whatever the main stream queues next
    if (c->lanes.marked & 1) c->lanes.marked &= ~1;  // the caller's mark (ndt_side_lanes_mark)
    else HIPCHK(c, hipEventRecord(c->lanes.ev_main_fit.get(), c->stream.get()));
    c->lanes.fit_worker->post([c, Tm, src, N, max_range, ctx_source]() -> ndt_status {
        HIPCHK(c, hipStreamWaitEvent(c->lanes.fit_stream.get(), c->lanes.ev_main_fit.get(), 0));
        // 16-lane team per query; the grid capped at 32 Ki workgroups (measured caps 8192 / 2048 / 1024 / 512 of 256-thread
        // workgroups: 89.4 / 85.9 / 90.7 / 128.9 us on C3)
        constexpr int grid_cap = 8192 * (256 / kFitBlock);
        const int nb = grid_for(N, kFitBlock / kFitTeam, grid_cap);
        const int ngrp = ceil_div(nb, kFitGroup);
        TRY(ensure(c, c->fit_sum, nb + ngrp)); TRY(ensure(c, c->fit_cnt, nb + ngrp)); TRY(ensure(c, c->fit_d2, N));
        const size_t n_ticket = (size_t)kFitTicketStride * (1 + ngrp);
        if (c->fit_ticket.cap < n_ticket) {
            TRY(ensure(c, c->fit_ticket, n_ticket));
            HIPCHK(c, hipMemsetAsync(c->fit_ticket.p, 0, c->fit_ticket.cap * sizeof(unsigned), c->lanes.fit_stream.get()));
        }
        // the last workgroup sums the partials and writes (sum, count) straight into the pinned result slots
        hipLaunchKernelGGL(k_fitness, dim3(nb), dim3(kFitBlock), 0, c->lanes.fit_stream.get(), src, N, Tm, c->fit_ix.hdr.p, c->fit_ix.blk.p,
                           c->fit_ix.off.p, c->fit_ix.pts.p, max_range, c->fit_d2.p, c->fit_sum.p, c->fit_cnt.p, c->fit_ticket.p,
                           &c->h_async->fit_sum, &c->h_async->fit_cnt);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->lanes.ev_fit.get(), c->lanes.fit_stream.get()));
        if (ctx_source) HIPCHK(c, hipEventRecord(c->lanes.ev_fit_src.get(), c->lanes.fit_stream.get()));
        return NDT_OK;
    });
    if (ctx_source) c->lanes.fit_src_used = true;
    c->lanes.fit_pending = true;
    c->fit_n = N;
    return NDT_OK;
}

}  // namespace ndt::host

extern "C" {

ndt_status ndt_fitness_score_async(ndt_ctx* c, const float* T, double max_range) {
    if (!c) return NDT_EINVAL;
    TRY(need_target_and_source(c));
    TRY(set_dev(c));
    TRY(flush_source(c));  // the query reads the ctx source on the fit lane, behind the main stream's work so far
    return fitness_enqueue(c, T, max_range, c->source.p, c->N, true);
}

ndt_status ndt_fitness_score_async_cloud(ndt_ctx* c, const float* T, double max_range, const float* d_src4, size_t n) {
    if (!c || (n && !d_src4) || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad fitness cloud");
    if (!c->has_target) return fail(c, NDT_ENOTARGET, "no input target");
    if (n == 0) return fail(c, NDT_ENOSOURCE, "empty fitness cloud");
    return fitness_enqueue(c, T, max_range, reinterpret_cast<const float4*>(d_src4), (int)n, false);
}

// getFitnessScore of the last align against the target it aligned to, callable after setInputTarget has replaced that
// target (odom_node.cpp:280 runs before :349; queuing the query after the new target's build lets the build's first
// kernels start before the query fills the CUs).  Needs that target's index queued (ndt_fitness_index_async after its
// setInputTarget); the query is queued ahead of the new target's index build on the fit lane (FIFO).
ndt_status ndt_fitness_score_async_aligned(ndt_ctx* c, double max_range, const float* d_src4, size_t n) {
    if (!c || (n && !d_src4) || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad fitness cloud");
    if (n == 0) return fail(c, NDT_ENOSOURCE, "empty fitness cloud");
    if (c->align_tgt_gen == ~0ull) return fail(c, NDT_EINVAL, "no align result");
    TRY(set_dev(c));
    if (c->align_tgt_gen == c->tgt_gen) {  // the target has not changed since the align
        float T[16];
        for (int k = 0; k < 16; ++k) T[k] = last_final(c)[k];
        return fitness_enqueue(c, T, max_range, reinterpret_cast<const float4*>(d_src4), (int)n, false);
    }
    if (c->fit_ix_gen != c->align_tgt_gen || !c->lanes.fit_worker || c->lanes.fit_worker->failed())
        return fail(c, NDT_EINVAL, "getFitnessScore: the aligned target's index was not queued before setInputTarget");
    float T[16];
    for (int k = 0; k < 16; ++k) T[k] = last_final(c)[k];
    return fitness_enqueue(c, T, max_range, reinterpret_cast<const float4*>(d_src4), (int)n, false, true);
}

ndt_status ndt_fitness_index_async(ndt_ctx* c) {
    if (!c) return NDT_EINVAL;
    if (!c->has_target) return fail(c, NDT_ENOTARGET, "no input target");
    TRY(set_dev(c));
    return ensure_fit_index(c);
}

ndt_status ndt_fitness_score_result(ndt_ctx* c, double* out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    std::string msg;
    // a failed fit-lane job is taken (and cleared) even when no query is pending, so that it cannot stay stuck
    const ndt_status st = c->lanes.fit_worker ? c->lanes.fit_worker->take_error(&msg) : NDT_OK;  // every fit-lane job issued
    if (st == NDT_OK && !c->lanes.fit_pending) return fail(c, NDT_EINVAL, "no fitness score enqueued");
    TRY(set_dev(c));
    if (st != NDT_OK) {
        c->lanes.fit_pending = false;
        c->fit_valid = false;  // the index may not have been built
        return fail(c, st, "getFitnessScore: " + msg);
    }
    HIPCHK(c, hipEventSynchronize(c->lanes.ev_fit.get()));
    const double sum = c->h_async->fit_sum;
    const long long cnt = c->h_async->fit_cnt;
    if (cnt < 0) {
        c->fit_valid = false;
        return fail(c, NDT_EDEVICE, "getFitnessScore: nearest-neighbour index sort: radix look-back timed out");
    }
    // Registration::getFitnessScore: mean of the squared distances <= max_range, DBL_MAX when none qualifies
    *out = cnt > 0 ? sum / (double)cnt : DBL_MAX;
    return NDT_OK;
}

ndt_status ndt_fitness_score(ndt_ctx* c, const float T[16], double max_range, double* out, float* nn_d2) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    TRY(ndt_fitness_score_async(c, T, max_range));
    if (nn_d2) {
        std::string msg;
        const ndt_status st = c->lanes.fit_worker->drain(&msg);  // the query has been issued (its failure is reported below)
        if (st == NDT_OK) {
            HIPCHK(c, hipMemcpyAsync(nn_d2, c->fit_d2.p, (size_t)c->fit_n * sizeof(float), hipMemcpyDeviceToHost, c->lanes.fit_stream.get()));
            HIPCHK(c, hipStreamSynchronize(c->lanes.fit_stream.get()));
        }
    }
    return ndt_fitness_score_result(c, out);
}

ndt_status ndt_keyframe_insert_async(ndt_ctx* c, const float T[16], const float* d_scan4, size_t n, float leaf, float* d_map_a, size_t n_a,
                                     float* d_map_b, size_t n_b) {
    if (!c || !T || (n && (!d_scan4 || !d_map_a || !d_map_b)) || !(leaf > 0.f) || n > 0x7fffffffULL)
        return fail(c, NDT_EINVAL, "bad keyframe insert args");
    TRY(set_dev(c));
    TRY(side_lanes(c));
    c->lanes.ins_n_in = n;
    c->lanes.ins_pending = true;
    // the insertion lane: behind the main stream's work so far (whatever wrote the scan or grew the maps; the marker is
    // recorded here, on the caller's thread), beside what the main stream queues next; its own binning header and sort
    // scratch, its launches issued by the lane's host thread
    hipEvent_t ev_main = c->lanes.ev_main_ins.get();
    if (c->lanes.marked & 2) {  // the caller's mark (ndt_side_lanes_mark)
        c->lanes.marked &= ~2;
        ev_main = c->lanes.ev_main_fit.get();
    } else {
        HIPCHK(c, hipEventRecord(c->lanes.ev_main_ins.get(), c->stream.get()));
    }
    Mat4f Tm;
    for (int k = 0; k < 16; ++k) Tm.m[k] = T[k];
    const float4* scan = reinterpret_cast<const float4*>(d_scan4);
    float4* dst_a = reinterpret_cast<float4*>(d_map_a) + n_a;
    float4* dst_b = reinterpret_cast<float4*>(d_map_b) + n_b;
    c->lanes.ins_worker->post([c, Tm, scan, n, leaf, dst_a, dst_b, ev_main]() -> ndt_status {
        if (n == 0) {
            HIPCHK(c, hipStreamSynchronize(c->lanes.ins_stream.get()));  // no earlier insertion still writes the pinned header
            std::memset(&c->h_async->ins_hdr, 0, sizeof(GridHeader));
            c->h_async->ins_hdr.empty = 1;
            HIPCHK(c, hipEventRecord(c->lanes.ev_ins.get(), c->lanes.ins_stream.get()));
            return NDT_OK;
        }
        const Lane L{c->lanes.ins_stream.get(), c->lanes.s_ins};
        HIPCHK(c, hipStreamWaitEvent(L.st, ev_main, 0));
        TRY(ensure(c, c->lanes.ins_tr, n)); TRY(ensure(c, c->lanes.ins_ds, n));
        hipLaunchKernelGGL(k_transform_mat, dim3(ceil_div((long long)n, kBlock)), dim3(kBlock), 0, L.st, scan, (int)n, Tm, c->lanes.ins_tr.p);
        TRY(enqueue_voxel_grid(c, L, c->lanes.ins_tr.p, (int)n, leaf, c->lanes.d_hdr_ins.p, c->lanes.ins_ds.p));
        hipLaunchKernelGGL(k_append2, dim3(grid_for((long long)n, kBlock, 1024)), dim3(kBlock), 0, L.st,
                           c->lanes.ins_ds.p, c->lanes.ins_tr.p, (int)n, c->lanes.d_hdr_ins.p, dst_a, dst_b);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&c->h_async->ins_hdr, c->lanes.d_hdr_ins.p, sizeof(GridHeader), hipMemcpyDeviceToHost, L.st));
        HIPCHK(c, hipEventRecord(c->lanes.ev_ins.get(), L.st));
        return NDT_OK;
    });
    return NDT_OK;
}

ndt_status ndt_side_lanes_mark(ndt_ctx* c) {
    if (!c) return NDT_EINVAL;
    TRY(set_dev(c));
    TRY(side_lanes(c));
    HIPCHK(c, hipEventRecord(c->lanes.ev_main_fit.get(), c->stream.get()));
    c->lanes.marked = 3;
    return NDT_OK;
}

ndt_status ndt_keyframe_insert_result(ndt_ctx* c, size_t* n_inserted) {
    if (!c || !n_inserted) return fail(c, NDT_EINVAL, "null argument");
    if (!c->lanes.ins_pending) return fail(c, NDT_EINVAL, "no keyframe insertion enqueued");
    TRY(set_dev(c));
    std::string msg;
    const ndt_status st = c->lanes.ins_worker->take_error(&msg);  // the insertion has been issued
    if (st != NDT_OK) {
        c->lanes.ins_pending = false;
        return fail(c, st, "keyframe insertion: " + msg);
    }
    HIPCHK(c, hipEventSynchronize(c->lanes.ev_ins.get()));
    const GridHeader& h = c->h_async->ins_hdr;
    if (h.pad[0]) return fail(c, NDT_EDEVICE, "keyframe insertion: VoxelGrid sort: radix look-back timed out");
    *n_inserted = h.overflow ? c->lanes.ins_n_in : (h.empty ? 0 : (size_t)h.n_leaves);
    return h.overflow ? NDT_EOVERFLOW : NDT_OK;
}

}  // extern "C"
