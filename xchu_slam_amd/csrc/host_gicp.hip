// host_gicp.hip — Generalized-ICP over the ctx's target and source (pclomp::GeneralizedIterativeClosestPoint): ndt_gicp_*.
#include "ndt_host.h"

// One round of launches between two reads of the state: kGicpRoundBlocks blocks of (k_gicp_pairs, kGicpBlockEvals x
// k_gicp_eval).  A launch whose phase is not the state's returns at its first load, so the sequence is fixed; a solve
// longer than one block's evaluations runs on through the next block, whose k_gicp_pairs launch returns at once.
// A round is one captured linear graph (no parallel branches), as the runs of passes of host_icp.hip.
// kGicpRoundBlocks is the measured choice (profiles/gicp.md); NDT_GICP_ROUND overrides it and NDT_GICP_GRAPH=0 issues
// the round as plain stream launches, for such A/B runs.
constexpr int kGicpBlockEvals = 15;
constexpr int kGicpRoundBlocks = 4;

static ndt_status gicp_params_ok(ndt_ctx* c, const ndt_gicp_params& p) {
    if (!(p.max_corr_dist >= 0.0) || !(p.trans_eps > 0.0) || !(p.rot_eps > 0.0) || !(p.gicp_epsilon > 0.0) || p.max_inner_iter < 1)
        return fail(c, NDT_EINVAL, "invalid GICP params");
    if (p.k_correspondences < 1 || p.k_correspondences > kGicpMaxK)
        return fail(c, NDT_EINVAL, "GICP: k_correspondences must be 1.." + std::to_string(kGicpMaxK));
    return NDT_OK;
}

static void launch_cov(ndt_ctx* c, const float4* pts, int n, const ndt_gicp_params& p, const NNIndex& ix, double* out, double* raw) {
    const int nb = grid_for(n, kGicpTeams, kGicpCovMaxBlocks);
    if (p.k_correspondences <= 20)
        hipLaunchKernelGGL(k_gicp_cov<20>, dim3(nb), dim3(kGicpBlock), 0, c->stream.get(), pts, n, p.k_correspondences, p.gicp_epsilon,
                           ix.hdr.p, ix.blk.p, ix.off.p, ix.pts.p, ix.idx.p, out, raw);
    else
        hipLaunchKernelGGL(k_gicp_cov<32>, dim3(nb), dim3(kGicpBlock), 0, c->stream.get(), pts, n, p.k_correspondences, p.gicp_epsilon,
                           ix.hdr.p, ix.blk.p, ix.off.p, ix.pts.p, ix.idx.p, out, raw);
}

// Covariances of the target (which = 0) or the source (1), kept until that cloud, k or epsilon changes (the reference
// resets them in setInputTarget / setInputSource).  raw: also the covariances before the SVD, always recomputed.
static ndt_status gicp_covariances(ndt_ctx* c, int which, const ndt_gicp_params& p, bool raw) {
    GicpRun& g = c->gicp;
    const int n = which == 0 ? c->M : c->N;
    if (n < p.k_correspondences)
        return fail(c, NDT_EINVAL, std::string("GICP: the ") + (which == 0 ? "target" : "source") + " has fewer points than k_correspondences");
    GicpRun::Cov& cv = which == 0 ? g.cov_tgt : g.cov_src;
    const unsigned long long gen = which == 0 ? c->tgt_gen : c->src_gen;
    if (!raw && cv.valid && cv.gen == gen && cv.k == p.k_correspondences && cv.eps == p.gicp_epsilon) return NDT_OK;
    cv.valid = false;
    TRY(ensure(c, cv.buf, (size_t)9 * n));
    if (raw) TRY(ensure(c, g.raw, (size_t)9 * n));
    if (which == 0) {
        TRY(target_nn_index(c, "GICP"));
        launch_cov(c, c->target_ptr, n, p, c->fit_ix, cv.buf.p, raw ? g.raw.p : nullptr);
    } else {
        TRY(ensure(c, g.src_ix.hdr, 1));
        TRY(enqueue_nn_index(c, main_lane(c), c->source.p, n, 1, c->prm.resolution, g.src_ix, true));
        launch_cov(c, c->source.p, n, p, g.src_ix, cv.buf.p, raw ? g.raw.p : nullptr);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));  // check_index_sort reads behind a synchronised stream
    TRY(check_index_sort(c, which == 0 ? c->fit_ix : g.src_ix, "GICP"));
    cv.valid = true;
    cv.gen = gen;
    cv.k = p.k_correspondences;
    cv.eps = p.gicp_epsilon;
    return NDT_OK;
}

static ndt_status gicp_buffers(ndt_ctx* c) {
    GicpRun& g = c->gicp;
    TRY(make_run_state(c, g.d_state, g.d_hist, kGicpMaxHistory, g.h_state, hipHostMallocDefault, "GICP state allocation failed"));
    const int N = c->N;
    TRY(ensure(c, g.match, N)); TRY(ensure(c, g.d2, N)); TRY(ensure(c, g.qt, N)); TRY(ensure(c, g.gp, N));
    TRY(ensure(c, g.M, (size_t)9 * N));
    TRY(ensure(c, g.part, (size_t)kGicpSums * kGicpEvalBlocks));
    if (!g.ticket.p) {
        TRY(ensure(c, g.ticket, 64));
        HIPCHK(c, hipMemsetAsync(g.ticket.p, 0, g.ticket.cap * sizeof(unsigned), c->stream.get()));
    }
    return NDT_OK;
}

static void launch_eval(ndt_ctx* c) {
    GicpRun& g = c->gicp;
    const int nb = grid_for(c->N, kGicpBlock, kGicpEvalBlocks);
    hipLaunchKernelGGL(k_gicp_eval, dim3(nb), dim3(kGicpBlock), 0, c->stream.get(), c->source.p, c->N, g.d_state.p, g.match.p, g.qt.p,
                       g.gp.p, g.M.p, g.part.p, g.ticket.p + 32, g.d_hist.p);
}

// one round: its launches and the read-back of the state into the pinned copy
static ndt_status gicp_round_body(ndt_ctx* c, int blocks, int nbp) {
    GicpRun& g = c->gicp;
    for (int b = 0; b < blocks; ++b) {
        hipLaunchKernelGGL(k_gicp_pairs, dim3(nbp), dim3(kGicpBlock), 0, c->stream.get(), c->source.p, c->N, g.d_state.p, c->fit_ix.hdr.p,
                           c->fit_ix.blk.p, c->fit_ix.off.p, c->fit_ix.pts.p, c->fit_ix.idx.p, g.cov_src.buf.p, g.cov_tgt.buf.p,
                           g.match.p, g.d2.p, g.qt.p, g.gp.p, g.M.p, g.ticket.p, g.d_hist.p);
        for (int e = 0; e < kGicpBlockEvals; ++e) launch_eval(c);
    }
    const hipError_t e = hipMemcpyAsync(&g.h_state[0], g.d_state.p, sizeof(GicpState), hipMemcpyDeviceToHost, c->stream.get());
    if (e != hipSuccess) return fail(c, NDT_EDEVICE, std::string("GICP round: ") + hipGetErrorString(e));
    return NDT_OK;
}

static ndt_status gicp_graph(ndt_ctx* c, int blocks, int nbp, hipGraphExec_t* out) {
    GicpRun& g = c->gicp;
    // the key names every buffer of the round that can be reallocated between aligns; d_state, d_hist, h_state, part
    // and ticket are allocated once per ctx, at fixed sizes (gicp_buffers), and never grow
    const auto a = [](const void* p) { return (long long)(uintptr_t)p; };
    const long long key[16] = {blocks, nbp, c->N, a(c->source.p), a(c->fit_ix.hdr.p), a(c->fit_ix.blk.p), a(c->fit_ix.off.p),
                               a(c->fit_ix.pts.p), a(c->fit_ix.idx.p), a(g.cov_src.buf.p), a(g.cov_tgt.buf.p), a(g.match.p),
                               a(g.d2.p), a(g.qt.p), a(g.gp.p), a(g.M.p)};
    return keyed_graph(c, g.graph, key, "GICP graph capture: ", [&]() -> ndt_status { return gicp_round_body(c, blocks, nbp); }, out);
}

extern "C" {

// Defaults of pclomp::GeneralizedIterativeClosestPoint's constructor (gicp_omp.h:108-118)
ndt_status ndt_gicp_default_params(ndt_gicp_params* out) {
    if (!out) return NDT_EINVAL;
    out->max_corr_dist = 5.0;
    out->max_iter = 200;
    out->trans_eps = 5e-4;
    out->rot_eps = 2e-3;
    out->k_correspondences = 20;
    out->gicp_epsilon = 1e-3;
    out->max_inner_iter = 20;
    return NDT_OK;
}

ndt_status ndt_gicp_align(ndt_ctx* c, const ndt_gicp_params* prm, const float guess[16], ndt_gicp_result* out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    ndt_gicp_params p;
    (void)ndt_gicp_default_params(&p);
    if (prm) p = *prm;
    TRY(gicp_params_ok(c, p));
    TRY(need_target_and_source(c));
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an asynchronous align is in flight (ndt_align_wait first)");
    TRY(set_dev(c));
    TRY(flush_source(c));
    GicpRun& g = c->gicp;
    g.n = 0;
    TRY(gicp_covariances(c, 0, p, false));
    TRY(gicp_covariances(c, 1, p, false));
    TRY(target_nn_index(c, "GICP"));  // a target unchanged since its covariances: the index may have been dropped since
    TRY(gicp_buffers(c));
    const int N = c->N;
    GicpState* s0 = &g.h_state[1];
    std::memset(s0, 0, sizeof(GicpState));
    s0->corr2 = p.max_corr_dist * p.max_corr_dist;
    s0->rot_eps = p.rot_eps;
    s0->trans_eps = p.trans_eps;
    s0->max_iter = p.max_iter;
    s0->max_inner = p.max_inner_iter;
    for (int k = 0; k < 16; ++k) s0->guess[k] = guess ? guess[k] : (k % 5 == 0 ? 1.f : 0.f);
    gicp_identity16(s0->trans);
    gicp_identity16(s0->prev);
    gicp_set_rtg(s0);
    gicp_set_final(s0);
    s0->phase = GICP_PAIRS;
    HIPCHK(c, hipMemcpyAsync(g.d_state.p, s0, sizeof(GicpState), hipMemcpyHostToDevice, c->stream.get()));
    const int nbp = grid_for(N, kGicpTeams, kGicpMaxBlocks);
    // the round budget: every block of a round that starts unfinished runs at least kGicpBlockEvals useful launches, or
    // ends a solve; an outer iteration takes at most one k_gicp_pairs and kGicpMaxEvals evaluations
    const long long iters = std::max(p.max_iter, 1);
    const long long blocks = iters * (kGicpMaxEvals + 1) / kGicpBlockEvals + 2 * iters + 2;
    static const int round_blocks = [] {
        const char* e = std::getenv("NDT_GICP_ROUND");  // A/B runs
        return e ? std::max(1, std::min(64, std::atoi(e))) : kGicpRoundBlocks;
    }();
    const long long max_rounds = blocks / round_blocks + 2;
    static const bool use_graph = [] {
        const char* e = std::getenv("NDT_GICP_GRAPH");  // A/B runs
        return !e || std::atoi(e) != 0;
    }();
    hipGraphExec_t gx = nullptr;
    if (use_graph) TRY(gicp_graph(c, round_blocks, nbp, &gx));
    c->have_result = false;
    bool finished = false;
    g.launches = 0;
    g.rounds = 0;
    for (long long round = 0; round < max_rounds && !finished; ++round) {
        if (gx) HIPCHK(c, hipGraphLaunch(gx, c->stream.get()));
        else TRY(gicp_round_body(c, round_blocks, nbp));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
        finished = g.h_state[0].phase == GICP_DONE;
        g.launches += round_blocks * (1 + kGicpBlockEvals);
        g.rounds += 1;
    }
    if (!finished) return fail(c, NDT_EDEVICE, "GICP did not finish within its round budget");
    TRY(check_index_sort(c, c->fit_ix, "GICP"));  // behind the last round's synchronise, which it relies on
    const GicpState& s = g.h_state[0];
    g.hist.resize(std::min(s.hist_count, kGicpMaxHistory));
    if (!g.hist.empty())
        HIPCHK(c, hipMemcpy(g.hist.data(), g.d_hist.p, g.hist.size() * sizeof(GicpRecordDev), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) {
        c->icp.final_tf[k] = s.final_tf[k];  // the last align of either point-to-point kind (last_final)
        out->final_tf[k] = s.final_tf[k];
    }
    out->converged = s.converged;
    out->state = s.conv_state;
    out->nr_iterations = s.iterations;
    out->f = s.f_last;
    out->n_pairs = s.pairs;
    out->n_evals = s.total_evals;
    g.n = N;
    g.src_gen = c->src_gen;
    c->icp.last = true;
    c->have_result = true;
    c->align_tgt_gen = c->tgt_gen;
    return NDT_OK;
}

ndt_status ndt_gicp_history(ndt_ctx* c, ndt_gicp_record* out, int cap, int* n_out) {
    if (!c || !n_out || (cap > 0 && !out)) return fail(c, NDT_EINVAL, "bad history args");
    const int n = std::min((int)c->gicp.hist.size(), std::max(cap, 0));
    for (int i = 0; i < n; ++i) {
        const GicpRecordDev& r = c->gicp.hist[i];
        for (int k = 0; k < 16; ++k) out[i].T[k] = r.T[k];
        out[i].n_pairs = r.pairs;
        out[i].f = r.f;
        out[i].inner_iterations = r.inner;
        out[i].n_evals = r.evals;
        out[i].min_status = r.status;
        out[i].delta = r.delta;
        out[i].state = r.conv_state;
    }
    *n_out = (int)c->gicp.hist.size();
    return NDT_OK;
}

ndt_status ndt_gicp_covariances(ndt_ctx* c, const ndt_gicp_params* prm, int which, int raw, double* out, size_t cap, size_t* n_out) {
    if (!c || !n_out || (which != 0 && which != 1)) return fail(c, NDT_EINVAL, "bad covariance args");
    ndt_gicp_params p;
    (void)ndt_gicp_default_params(&p);
    if (prm) p = *prm;
    TRY(gicp_params_ok(c, p));
    if (which == 0 && !c->has_target) return fail(c, NDT_ENOTARGET, "no input target");
    if (which == 1 && (!c->has_source || c->N == 0)) return fail(c, NDT_ENOSOURCE, "no input source");
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an asynchronous align is in flight (ndt_align_wait first)");
    TRY(set_dev(c));
    if (which == 1) TRY(flush_source(c));
    TRY(gicp_covariances(c, which, p, raw != 0));
    const size_t n = (size_t)(which == 0 ? c->M : c->N);
    const size_t m = std::min(n, cap);
    const double* src = raw ? c->gicp.raw.p : (which == 0 ? c->gicp.cov_tgt.buf.p : c->gicp.cov_src.buf.p);
    if (out && m) HIPCHK(c, hipMemcpy(out, src, m * 9 * sizeof(double), hipMemcpyDeviceToHost));
    *n_out = n;
    return NDT_OK;
}

ndt_status ndt_gicp_correspondences(ndt_ctx* c, int* index, float* d2, double* M9, size_t cap, size_t* n_out) {
    if (!c || !n_out) return fail(c, NDT_EINVAL, "null argument");
    if (!c->gicp.n || !c->gicp.match.p || c->gicp.src_gen != c->src_gen) return fail(c, NDT_EINVAL, "no GICP align over the current source");
    TRY(set_dev(c));
    const size_t n = std::min((size_t)c->gicp.n, cap);
    if (index && n) HIPCHK(c, hipMemcpy(index, c->gicp.match.p, n * sizeof(int), hipMemcpyDeviceToHost));
    if (d2 && n) HIPCHK(c, hipMemcpy(d2, c->gicp.d2.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (M9 && n) HIPCHK(c, hipMemcpy(M9, c->gicp.M.p, n * 9 * sizeof(double), hipMemcpyDeviceToHost));
    *n_out = (size_t)c->gicp.n;
    return NDT_OK;
}

ndt_status ndt_gicp_evaluate(ndt_ctx* c, const double x[6], double* f, double g6[6]) {
    if (!c || !x || !f || !g6) return fail(c, NDT_EINVAL, "null argument");
    GicpRun& g = c->gicp;
    if (!g.n || g.n != c->N || g.src_gen != c->src_gen || !g.h_state) return fail(c, NDT_EINVAL, "no GICP align over the current source");
    if (g.h_state[0].pairs < 1) return fail(c, NDT_EINVAL, "the last GICP iteration has no pairs");
    TRY(set_dev(c));
    GicpState* s = &g.h_state[1];
    *s = g.h_state[0];
    s->phase = GICP_EVAL_ONLY;
    for (int k = 0; k < 6; ++k) s->min.x[k] = x[k];
    gicp_apply_state(s->guess, s->min.x, s->T_trial);
    HIPCHK(c, hipMemcpyAsync(g.d_state.p, s, sizeof(GicpState), hipMemcpyHostToDevice, c->stream.get()));
    launch_eval(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s, g.d_state.p, sizeof(GicpState), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    *f = s->ev_f;
    for (int k = 0; k < 6; ++k) g6[k] = s->ev_g[k];
    return NDT_OK;
}

ndt_status ndt_gicp_run_stats(ndt_ctx* c, int* launches, int* rounds) {
    if (!c || !launches || !rounds) return fail(c, NDT_EINVAL, "null argument");
    *launches = c->gicp.launches;
    *rounds = c->gicp.rounds;
    return NDT_OK;
}

}  // extern "C"
