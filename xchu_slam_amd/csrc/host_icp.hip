// host_icp.hip — point-to-point ICP over the ctx's target and source (pgo_node's ICPRefine): ndt_icp_*.
#include "ndt_host.h"

// Passes per graph launch (one state read-back per run).  A run past the converged iteration costs one empty launch per
// leftover pass (each returns at its first load), a shorter run one host round trip more per run.  Measured on the
// MI355X with the loop-sized pair of DESIGN.md §4 (15 k points against 163 k, pgo_node's settings, 21 iterations):
// whole align 1.48 / 1.29 / 1.19 / 1.14 / 1.14 ms at runs of 1 / 2 / 4 / 8 / 16 passes (host wall time, medians of
// three interleaved repeats, profiles/icp_loop_pair.md): 8 is the shortest run at the floor.
// NDT_ICP_RUN overrides it for such A/B runs.
constexpr int kIcpRun = 8;

static ndt_status icp_graph(ndt_ctx* c, int run, int nb, hipGraphExec_t* out) {
    const long long key[12] = {run, nb, c->N, (long long)(uintptr_t)c->icp.x.p, (long long)(uintptr_t)c->fit_ix.blk.p,
                               (long long)(uintptr_t)c->fit_ix.off.p, (long long)(uintptr_t)c->fit_ix.pts.p,
                               (long long)(uintptr_t)c->fit_ix.idx.p, (long long)(uintptr_t)c->icp.match.p,
                               (long long)(uintptr_t)c->icp.d2.p, (long long)(uintptr_t)c->icp.part.p,
                               (long long)(uintptr_t)c->icp.ticket.p};
    return keyed_graph(c, c->icp.graph, key, "ICP graph capture: ", [&]() -> ndt_status {
        for (int k = 0; k < run; ++k)
            hipLaunchKernelGGL(k_icp_pass, dim3(nb), dim3(kIcpBlock), 0, c->stream.get(), c->icp.x.p, c->N, c->icp.d_state.p, c->fit_ix.hdr.p, c->fit_ix.blk.p,
                               c->fit_ix.off.p, c->fit_ix.pts.p, c->fit_ix.idx.p, c->icp.match.p, c->icp.d2.p, c->icp.part.p,
                               c->icp.ticket.p, c->icp.d_hist.p);
        const hipError_t e = hipMemcpyAsync(&c->icp.h_state[0], c->icp.d_state.p, sizeof(IcpState), hipMemcpyDeviceToHost, c->stream.get());
        if (e != hipSuccess) return fail(c, NDT_EDEVICE, std::string("ICP graph capture: ") + hipGetErrorString(e));
        return NDT_OK;
    }, out);
}

extern "C" {

// ================================================================ point-to-point ICP (pgo_node's ICPRefine)
// Defaults of pcl::Registration / pcl::IterativeClosestPoint (PCL 1.7): 10 iterations, sqrt(DBL_MAX) correspondence
// distance, both epsilons 0 (an epsilon of 0 switches its test off).
ndt_status ndt_icp_default_params(ndt_icp_params* out) {
    if (!out) return NDT_EINVAL;
    out->max_corr_dist = std::sqrt(DBL_MAX);
    out->max_iter = 10;
    out->trans_eps = 0.0;
    out->fit_eps = 0.0;
    return NDT_OK;
}

// pcl::IterativeClosestPoint::align(output, guess) (pgo_node.cpp:462) over the ctx's target and source.
ndt_status ndt_icp_align(ndt_ctx* c, const ndt_icp_params* prm, const float guess[16], ndt_icp_result* out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    ndt_icp_params p;
    (void)ndt_icp_default_params(&p);
    if (prm) p = *prm;
    if (!(p.max_corr_dist >= 0.0) || !(p.trans_eps >= 0.0) || !(p.fit_eps >= 0.0)) return fail(c, NDT_EINVAL, "invalid ICP params");
    TRY(need_target_and_source(c));
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an asynchronous align is in flight (ndt_align_wait first)");
    TRY(set_dev(c));
    TRY(flush_source(c));
    TRY(target_nn_index(c, "ICP"));  // getFitnessScore's index, with the points' original indices from now on
    TRY(make_run_state(c, c->icp.d_state, c->icp.d_hist, kIcpMaxHistory, c->icp.h_state, hipHostMallocCoherent,
                       "ICP state allocation failed"));
    const int N = c->N;
    const int nb = grid_for(N, kIcpTeams, kIcpMaxBlocks);
    TRY(ensure(c, c->icp.x, N)); TRY(ensure(c, c->icp.match, N)); TRY(ensure(c, c->icp.d2, N));
    TRY(ensure(c, c->icp.part, (size_t)kIcpSums * kIcpMaxBlocks));
    if (!c->icp.ticket.p) {
        TRY(ensure(c, c->icp.ticket, 64));
        HIPCHK(c, hipMemsetAsync(c->icp.ticket.p, 0, c->icp.ticket.cap * sizeof(unsigned), c->stream.get()));
    }
    // X = the source (transformed by the guess in the first pass, unless the guess is the identity)
    TRY(copy16(c, c->stream.get(), c->icp.x.p, c->source.p, (size_t)N * sizeof(float4)));
    IcpState* s0 = &c->icp.h_state[1];
    std::memset(s0, 0, sizeof(IcpState));
    s0->max_corr2 = p.max_corr_dist * p.max_corr_dist;
    s0->trans_eps = p.trans_eps;
    s0->fit_eps = p.fit_eps;
    s0->max_iter = p.max_iter;
    s0->min_pairs = 3;
    s0->prev_mse = DBL_MAX;
    bool identity = true;
    for (int k = 0; k < 16; ++k) {
        const float v = guess ? guess[k] : (k % 5 == 0 ? 1.f : 0.f);
        s0->T[k] = v;
        s0->final_tf[k] = v;
        identity = identity && v == (k % 5 == 0 ? 1.f : 0.f);
    }
    s0->apply = identity ? 0 : 1;
    HIPCHK(c, hipMemcpyAsync(c->icp.d_state.p, s0, sizeof(IcpState), hipMemcpyHostToDevice, c->stream.get()));
    static const int run_env = [] {
        const char* e = std::getenv("NDT_ICP_RUN");  // A/B runs
        return e ? std::max(1, std::min(64, std::atoi(e))) : kIcpRun;
    }();
    const int run = run_env;
    hipGraphExec_t gx = nullptr;
    TRY(icp_graph(c, run, nb, &gx));
    const int max_rounds = std::max(p.max_iter, 1) / run + 2;
    Event e0, e1;  // profiling: timing events around the rounds, released on every return
    if (c->opt.profiling) {
        TRY(make_event(c, e0, hipEventDefault));
        TRY(make_event(c, e1, hipEventDefault));
        HIPCHK(c, hipEventRecord(e0.get(), c->stream.get()));
    }
    c->have_result = false;
    bool finished = false;
    for (int round = 0; round < max_rounds && !finished; ++round) {
        HIPCHK(c, hipGraphLaunch(gx, c->stream.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
        finished = c->icp.h_state[0].done != 0;
    }
    if (e0) {
        HIPCHK(c, hipEventRecord(e1.get(), c->stream.get()));
        HIPCHK(c, hipEventSynchronize(e1.get()));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, e0.get(), e1.get()));
        c->ms_align = ms;
    }
    if (!finished) return fail(c, NDT_EDEVICE, "ICP did not finish within its iteration budget");
    TRY(check_index_sort(c, c->fit_ix, "ICP"));  // behind the last round's synchronise, which it relies on
    const IcpState& s = c->icp.h_state[0];
    c->icp.hist.resize(std::min(s.hist_count, kIcpMaxHistory));
    if (!c->icp.hist.empty())
        HIPCHK(c, hipMemcpy(c->icp.hist.data(), c->icp.d_hist.p, c->icp.hist.size() * sizeof(IcpRecordDev), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) {
        c->icp.final_tf[k] = s.final_tf[k];
        out->final_tf[k] = s.final_tf[k];
    }
    out->converged = s.converged;
    out->state = s.conv_state;
    out->nr_iterations = s.iterations;
    out->mse = s.mse;
    out->n_pairs = s.pairs;
    c->icp.n = N;
    c->icp.last = true;
    c->have_result = true;
    c->align_tgt_gen = c->tgt_gen;
    return NDT_OK;
}

ndt_status ndt_icp_history(ndt_ctx* c, ndt_icp_record* out, int cap, int* n_out) {
    if (!c || !n_out || (cap > 0 && !out)) return fail(c, NDT_EINVAL, "bad history args");
    const int n = std::min((int)c->icp.hist.size(), std::max(cap, 0));
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 16; ++k) out[i].T[k] = c->icp.hist[i].T[k];
        out[i].n_pairs = c->icp.hist[i].pairs;
        out[i].mse = c->icp.hist[i].mse;
        out[i].state = c->icp.hist[i].conv_state;
    }
    *n_out = (int)c->icp.hist.size();
    return NDT_OK;
}

ndt_status ndt_icp_correspondences(ndt_ctx* c, int* index, float* d2, size_t cap, size_t* n_out) {
    if (!c || !n_out) return fail(c, NDT_EINVAL, "null argument");
    if (!c->icp.n || !c->icp.match.p) return fail(c, NDT_EINVAL, "no ICP align");
    TRY(set_dev(c));
    const size_t n = std::min((size_t)c->icp.n, cap);
    if (index && n) HIPCHK(c, hipMemcpy(index, c->icp.match.p, n * sizeof(int), hipMemcpyDeviceToHost));
    if (d2 && n) HIPCHK(c, hipMemcpy(d2, c->icp.d2.p, n * sizeof(float), hipMemcpyDeviceToHost));
    *n_out = (size_t)c->icp.n;
    return NDT_OK;
}

}  // extern "C"
