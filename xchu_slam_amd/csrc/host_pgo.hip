// host_pgo.hip — the pose graph on a ctx (pgo_node's GTSAM back end as a batch problem): ndt_pgo_*.
// The host keeps the graph (a few hundred KB at KITTI-00's 1541 keyframes) and the estimate; ndt_pgo_optimize uploads
// them, runs the whole optimisation as one launch on the ctx stream and reads the result back once.  Under
// NDT_PGO_SOLVER_DIRECT (ndt_pgo_set_solver) an outer iteration is a fixed sequence of launches instead
// (posegraph_direct.hip) and the host reads a small status block after each.
#include "ndt_host.h"
#include "ndt_pgo_schur.h"

struct ndt_pgo {
    ndt_ctx* c = nullptr;
    ndt_pgo_params prm{};
    std::vector<double> X, Zc;              // [n][12]: the estimate; the prior pose (node 0) / the odometry measurements
    std::vector<double> given_last;         // the last node's pose as given (the next odometry edge starts from it)
    std::vector<int> li, lj;
    std::vector<double> Zl, lvar, lk;
    std::vector<int> pnode;                 // position factors: the node; [7] measured xyz, variances, robust k
    std::vector<double> pf;
    DevBuf<double> d_f64;
    DevBuf<int> d_i32;
    DevBuf<ndt_pgo_record> d_hist;
    DevBuf<PgoOut> d_out;
    int solver = NDT_PGO_SOLVER_CG;
    DevBuf<double> d_dir, d_S;              // the direct solve: Kw and C; the dense matrix (grows, never shrinks)
    DevBuf<PgoDirectState> d_st;
    ndt_pgo_solver_stats_t stats{};          // of the last optimise
    std::vector<ndt_pgo_record> hist;       // of the last optimise
    std::vector<double> weights;            // of the last optimise (between factors)
    std::vector<double> pweights;           // of the last optimise (position factors)
};

// column-major 4 x 4 -> R row-major, t; false when it is not a finite rigid transform
static bool pgo_read_pose(const double* m, double* P) {
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(m[i])) return false;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[3 * r + c] = m[4 * c + r];
        P[9 + r] = m[12 + r];
    }
    double RtR[9];
    m3_tmul(P, P, RtR);
    for (int i = 0; i < 9; ++i)
        if (std::fabs(RtR[i] - (i % 4 == 0 ? 1.0 : 0.0)) > 1e-6) return false;
    const double det = P[0] * (P[4] * P[8] - P[5] * P[7]) - P[1] * (P[3] * P[8] - P[5] * P[6]) + P[2] * (P[3] * P[7] - P[4] * P[6]);
    return det > 0.0;
}

static bool pgo_valid_params(const ndt_pgo_params* p) {
    if (!p || p->max_iter < 1 || p->max_iter > kPgoMaxIter || p->cg_max_iter < 1 || p->cg_max_iter > kPgoMaxIter) return false;
    if (!(p->step_eps >= 0.0) || !(p->cg_rtol >= 0.0) || !std::isfinite(p->step_eps) || !std::isfinite(p->cg_rtol)) return false;
    for (int i = 0; i < 6; ++i)
        if (!(p->prior_var[i] > 0.0) || !(p->odom_var[i] > 0.0) || !std::isfinite(p->prior_var[i]) || !std::isfinite(p->odom_var[i])) return false;
    return true;
}

// The direct solve's outer iterations on the ctx stream (the inputs are already uploaded): the linearisation at the input,
// then per iteration the Schur build, the factorisation with b carried along, the back substitution and the step fused
// with the next linearisation; the status block is read after each and decides whether another is enqueued.
static ndt_status pgo_run_direct(ndt_pgo* g, const PgoGraph& d, const PgoArgs& a, PgoOut* o) {
    ndt_ctx* c = g->c;
    hipStream_t st = c->stream.get();
    const size_t n = (size_t)d.n, dim = 6 * (size_t)d.m + 3 * (size_t)d.np;
    PgoDirect dg;
    dg.d = (int)dim;
    dg.dp = (int)((dim + kPgoDirectTile - 1) / kPgoDirectTile) * kPgoDirectTile;
    TRY(ensure(c, g->d_dir, 6 * dim + 36 * n));
    TRY(ensure(c, g->d_S, ((size_t)dg.dp + 1) * (size_t)dg.dp));
    TRY(ensure(c, g->d_st, 1));
    dg.kw = g->d_dir.p;
    dg.C = dg.kw + 6 * dim;
    dg.S = g->d_S.p;
    dg.st = g->d_st.p;
    HIPCHK(c, hipMemsetAsync(dg.st, 0, sizeof(PgoDirectState), st));
    const int nt = dg.dp / kPgoDirectTile, nfb = (d.m + d.np + 15) / 16;
    PgoDirectState h;
    int factorizations = 0;
    for (int first = 1;; first = 0) {
        hipLaunchKernelGGL(k_pgo_direct_step, dim3(1), dim3(kPgoBlock), 0, st, d, a, dg, first);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&h, dg.st, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (h.done) break;
        if (dg.d == 0) continue;
        hipLaunchKernelGGL(k_pgo_schur, dim3(nfb, nfb), dim3(256), 0, st, d, dg);
        for (int kt = 0; kt < nt; ++kt) {
            hipLaunchKernelGGL(k_pgo_chol_diag, dim3(1), dim3(256), 0, st, dg, kt);
            hipLaunchKernelGGL(k_pgo_chol_panel, dim3(nt - kt), dim3(256), 0, st, dg, kt);
            if (kt + 1 < nt) hipLaunchKernelGGL(k_pgo_chol_trail, dim3(nt - kt - 1, nt - kt), dim3(256), 0, st, dg, kt);
        }
        hipLaunchKernelGGL(k_pgo_chol_back, dim3(1), dim3(256), 0, st, dg);
        HIPCHK(c, hipGetLastError());
        ++factorizations;
    }
    // as under CG: set once the launches ran, whatever status they report; a HIP error leaves the earlier optimise's
    g->stats = ndt_pgo_solver_stats_t{NDT_PGO_SOLVER_DIRECT, dg.d, kPgoDirectTile, factorizations, 0};
    o->status = h.status;
    o->bad = h.bad;
    o->iterations = h.iterations;
    o->converged = h.converged;
    o->cg_iterations = 0;
    o->cost0 = h.cost0;
    o->cost = h.cost;
    o->max_step = h.max_step;
    return NDT_OK;
}

extern "C" {

ndt_status ndt_pgo_set_solver(ndt_pgo* g, int solver) {
    if (!g) return NDT_EINVAL;
    if (solver != NDT_PGO_SOLVER_CG && solver != NDT_PGO_SOLVER_DIRECT)
        return fail(g->c, NDT_EINVAL, "unknown pose-graph solver " + std::to_string(solver) + " (0: CG, 1: direct)");
    g->solver = solver;
    return NDT_OK;
}

int ndt_pgo_get_solver(const ndt_pgo* g) { return g ? g->solver : -1; }

ndt_status ndt_pgo_solver_stats(ndt_pgo* g, ndt_pgo_solver_stats_t* out) {
    if (!g) return NDT_EINVAL;
    if (!out) return fail(g->c, NDT_EINVAL, "null argument");
    *out = g->stats;
    return NDT_OK;
}

// pgo_node's constants (pgo_node.cpp:85-93: prior 1e-12 x 6, odometry 1e-6 x 3 (rotation), 1e-4 x 3 (translation)).
// step_eps 1e-10 (rad, m) and cg_rtol 1e-10 are this library's: the reweighted iteration converges linearly, so the
// estimate is within a few step_eps of the stationary point; cg_rtol bounds each step's relative error far below that.
ndt_status ndt_pgo_default_params(ndt_pgo_params* out) {
    if (!out) return NDT_EINVAL;
    out->max_iter = 200;
    out->step_eps = 1e-10;
    out->cg_max_iter = 500;
    out->cg_rtol = 1e-10;
    for (int i = 0; i < 6; ++i) {
        out->prior_var[i] = 1e-12;
        out->odom_var[i] = i < 3 ? 1e-6 : 1e-4;
    }
    return NDT_OK;
}

ndt_status ndt_pgo_create(ndt_ctx* c, const ndt_pgo_params* prm, ndt_pgo** out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    *out = nullptr;
    ndt_pgo_params p;
    (void)ndt_pgo_default_params(&p);
    if (prm) p = *prm;
    if (!pgo_valid_params(&p)) return fail(c, NDT_EINVAL, "invalid pose-graph params");
    ndt_pgo* g = new ndt_pgo();
    g->c = c;
    g->prm = p;
    *out = g;
    return NDT_OK;
}

void ndt_pgo_destroy(ndt_pgo* g) {
    if (!g) return;
    drain_for_destroy(g->c);
    delete g;
}

int ndt_pgo_size(const ndt_pgo* g) { return g ? (int)(g->X.size() / 12) : -1; }

ndt_status ndt_pgo_add_node(ndt_pgo* g, const double pose[16], int* index) {
    if (!g) return NDT_EINVAL;
    if (!pose) return fail(g->c, NDT_EINVAL, "null argument");
    double P[12];
    if (!pgo_read_pose(pose, P)) return fail(g->c, NDT_EINVAL, "pose is not a finite rigid transform");
    const int k = ndt_pgo_size(g);
    double Z[12];
    if (k == 0)
        std::memcpy(Z, P, sizeof Z);  // the prior's mean
    else
        pose_inv_mul(g->given_last.data(), P, Z);
    g->X.insert(g->X.end(), P, P + 12);
    g->Zc.insert(g->Zc.end(), Z, Z + 12);
    g->given_last.assign(P, P + 12);
    if (index) *index = k;
    return NDT_OK;
}

// Host state only: the estimate of one node.  The factors keep the poses they were built from (Zc, given_last).
ndt_status ndt_pgo_set_estimate(ndt_pgo* g, int node, const double pose[16]) {
    if (!g) return NDT_EINVAL;
    if (!pose) return fail(g->c, NDT_EINVAL, "null argument");
    if (node < 0 || node >= ndt_pgo_size(g)) return fail(g->c, NDT_EINVAL, "set estimate: node index out of range");
    double P[12];
    if (!pgo_read_pose(pose, P)) return fail(g->c, NDT_EINVAL, "pose is not a finite rigid transform");
    std::copy(P, P + 12, g->X.begin() + 12 * (size_t)node);
    return NDT_OK;
}

ndt_status ndt_pgo_add_between(ndt_pgo* g, int i, int j, const double Z[16], const double var[6], double robust_k) {
    if (!g) return NDT_EINVAL;
    ndt_ctx* c = g->c;
    if (!Z || !var) return fail(c, NDT_EINVAL, "null argument");
    const int n = ndt_pgo_size(g);
    if (i < 0 || j < 0 || i >= n || j >= n) return fail(c, NDT_EINVAL, "between factor: node index out of range");
    if (i == j) return fail(c, NDT_EINVAL, "between factor: i == j");
    double P[12];
    if (!pgo_read_pose(Z, P)) return fail(c, NDT_EINVAL, "between factor: measurement is not a finite rigid transform");
    for (int a = 0; a < 6; ++a)
        if (!(var[a] > 0.0) || !std::isfinite(var[a])) return fail(c, NDT_EINVAL, "between factor: variances must be positive and finite");
    if (!(robust_k >= 0.0) || !std::isfinite(robust_k)) return fail(c, NDT_EINVAL, "between factor: robust k must be >= 0");
    g->li.push_back(i);
    g->lj.push_back(j);
    g->Zl.insert(g->Zl.end(), P, P + 12);
    g->lvar.insert(g->lvar.end(), var, var + 6);
    g->lk.push_back(robust_k);
    return NDT_OK;
}

ndt_status ndt_pgo_add_position(ndt_pgo* g, int node, const double xyz[3], const double var[3], double robust_k) {
    if (!g) return NDT_EINVAL;
    ndt_ctx* c = g->c;
    if (!xyz || !var) return fail(c, NDT_EINVAL, "null argument");
    if (node < 0 || node >= ndt_pgo_size(g)) return fail(c, NDT_EINVAL, "position factor: node index out of range");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(xyz[a])) return fail(c, NDT_EINVAL, "position factor: position is not finite");
    for (int a = 0; a < 3; ++a)
        if (!(var[a] > 0.0) || !std::isfinite(var[a])) return fail(c, NDT_EINVAL, "position factor: variances must be positive and finite");
    if (!(robust_k >= 0.0) || !std::isfinite(robust_k)) return fail(c, NDT_EINVAL, "position factor: robust k must be >= 0");
    g->pnode.push_back(node);
    g->pf.insert(g->pf.end(), xyz, xyz + 3);
    g->pf.insert(g->pf.end(), var, var + 3);
    g->pf.push_back(robust_k);
    return NDT_OK;
}

ndt_status ndt_pgo_optimize(ndt_pgo* g, ndt_pgo_result* out) {
    if (!g) return NDT_EINVAL;
    ndt_ctx* c = g->c;
    if (!out) return fail(c, NDT_EINVAL, "null argument");
    const size_t n = (size_t)ndt_pgo_size(g), m = g->li.size(), np = g->pnode.size();
    if (n == 0) return fail(c, NDT_EINVAL, "the pose graph has no node");
    if (m > 0x3fffffffULL / 36 || n > 0x3fffffffULL / 18 || np > 0x3fffffffULL / 14) return fail(c, NDT_EINVAL, "pose graph too large");
    const bool direct = g->solver == NDT_PGO_SOLVER_DIRECT;
    const size_t dim = 6 * m + 3 * np;
    if (direct && dim > (size_t)kPgoDirectMaxDim)
        return fail(c, NDT_EINVAL, "direct solve: d = 6 m + 3 np = " + std::to_string(dim) + " is over the limit of " +
                                       std::to_string(kPgoDirectMaxDim) + "; the estimate is unchanged");
    TRY(set_dev(c));
    // per-node lists of loop edges (2 * edge + side), edges in insertion order; the position factors' slots by node
    std::vector<int> ints(2 * m + n + 1 + 2 * m + n + 1 + np, 0);
    int* h_li = ints.data();
    int* h_lj = h_li + m;
    int* h_off = h_lj + m;
    int* h_ent = h_off + n + 1;
    for (size_t q = 0; q < m; ++q) {
        h_li[q] = g->li[q];
        h_lj[q] = g->lj[q];
        ++h_off[g->li[q] + 1];
        ++h_off[g->lj[q] + 1];
    }
    for (size_t k = 0; k < n; ++k) h_off[k + 1] += h_off[k];
    {
        std::vector<int> fill(h_off, h_off + n);
        for (size_t q = 0; q < m; ++q) {
            h_ent[fill[g->li[q]]++] = (int)(2 * q);
            h_ent[fill[g->lj[q]]++] = (int)(2 * q + 1);
        }
    }
    int* h_poff = h_ent + 2 * m;
    int* h_pnode = h_poff + n + 1;
    std::vector<int> slot(np);  // of each position factor: by node, a node's in insertion order
    for (size_t q = 0; q < np; ++q) ++h_poff[g->pnode[q] + 1];
    for (size_t k = 0; k < n; ++k) h_poff[k + 1] += h_poff[k];
    {
        std::vector<int> fill(h_poff, h_poff + n);
        for (size_t q = 0; q < np; ++q) {
            slot[q] = fill[g->pnode[q]]++;
            h_pnode[slot[q]] = g->pnode[q];
        }
    }
    // inputs, contiguous: X, Zc, Zl, lvar, lk, the position factors by slot; then the work arrays
    const size_t n_in = 24 * n + 19 * m + 7 * np;
    const size_t n_f64 = n_in + 12 * n + 18 * n + 6 * n * 7 + 36 * m + 6 * m * 2 + m + 7 * np;
    std::vector<double> in;
    in.reserve(n_in);
    in.insert(in.end(), g->X.begin(), g->X.end());
    in.insert(in.end(), g->Zc.begin(), g->Zc.end());
    in.insert(in.end(), g->Zl.begin(), g->Zl.end());
    in.insert(in.end(), g->lvar.begin(), g->lvar.end());
    in.insert(in.end(), g->lk.begin(), g->lk.end());
    in.resize(n_in);
    for (size_t q = 0; q < np; ++q) std::copy_n(g->pf.data() + 7 * q, 7, in.data() + n_in - 7 * np + 7 * (size_t)slot[q]);
    TRY(ensure(c, g->d_f64, n_f64));
    TRY(ensure(c, g->d_i32, ints.size()));
    TRY(ensure(c, g->d_hist, (size_t)g->prm.max_iter + 1));
    TRY(ensure(c, g->d_out, 1));
    HIPCHK(c, hipMemcpyAsync(g->d_f64.p, in.data(), n_in * sizeof(double), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipMemcpyAsync(g->d_i32.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipMemsetAsync(g->d_out.p, 0, sizeof(PgoOut), c->stream.get()));
    PgoGraph d;
    d.n = (int)n;
    d.m = (int)m;
    d.np = (int)np;
    double* f = g->d_f64.p;
    auto take = [&f](size_t count) {
        double* p = f;
        f += count;
        return p;
    };
    d.X = take(12 * n);
    d.Zc = take(12 * n);
    d.Zl = take(12 * m);
    d.lvar = take(6 * m);
    d.lk = take(m);
    d.pf = take(7 * np);
    double* const d_pwork = take(7 * np);
    d.Xprev = take(12 * n);
    d.Jc = take(18 * n);
    d.rc = take(6 * n);
    d.z = take(6 * n);
    d.tmp = take(6 * n);
    d.y = take(6 * n);
    d.r = take(6 * n);
    d.p = take(6 * n);
    d.hp = take(6 * n);
    d.N = take(36 * m);
    d.bv = take(6 * m);
    d.dl = take(6 * m);
    d.w = take(m);
    d.li = g->d_i32.p;
    d.lj = d.li + m;
    d.off = d.lj + m;
    d.ent = d.off + n + 1;
    d.poff = d.ent + 2 * m;
    d.hist = g->d_hist.p;
    d.out = g->d_out.p;
    PgoArgs a;
    a.max_iter = g->prm.max_iter;
    a.cg_max_iter = g->prm.cg_max_iter;
    a.step_eps = g->prm.step_eps;
    a.cg_rtol = g->prm.cg_rtol;
    for (int i = 0; i < 6; ++i) {
        a.sig_prior[i] = std::sqrt(g->prm.prior_var[i]);
        a.sig_odom[i] = std::sqrt(g->prm.odom_var[i]);
    }
    PgoOut o;
    if (direct) {
        TRY(pgo_run_direct(g, d, a, &o));
    } else {
        hipLaunchKernelGGL(k_pgo_optimize, dim3(1), dim3(kPgoBlock), 0, c->stream.get(), d, a);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&o, g->d_out.p, sizeof o, hipMemcpyDeviceToHost, c->stream.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
        g->stats = ndt_pgo_solver_stats_t{NDT_PGO_SOLVER_CG, (int)std::min<size_t>(dim, 0x7fffffff), 0, 0, 0};
    }
    if (o.status == kPgoNearPi) {
        const std::string what = o.bad == 0 ? "the prior" : o.bad < (int)n ? "odometry edge " + std::to_string(o.bad - 1) + " -> " + std::to_string(o.bad)
                                                                            : "between factor " + std::to_string(o.bad - (int)n);
        return fail(c, NDT_EINVAL, "residual rotation within 1e-6 of pi at " + what + "; the estimate is unchanged");
    }
    if (o.status != kPgoOk) return fail(c, NDT_EOVERFLOW, "the optimisation left the finite range; the estimate is unchanged");
    g->hist.resize((size_t)o.iterations);
    g->weights.resize(m);
    g->pweights.resize(np);
    HIPCHK(c, hipMemcpy(g->X.data(), d.X, 12 * n * sizeof(double), hipMemcpyDeviceToHost));
    if (m) HIPCHK(c, hipMemcpy(g->weights.data(), d.w, m * sizeof(double), hipMemcpyDeviceToHost));
    if (np) {
        std::vector<double> work(7 * np);
        HIPCHK(c, hipMemcpy(work.data(), d_pwork, 7 * np * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < np; ++q) g->pweights[q] = work[7 * (size_t)slot[q] + 6];
    }
    if (o.iterations) HIPCHK(c, hipMemcpy(g->hist.data(), d.hist, (size_t)o.iterations * sizeof(ndt_pgo_record), hipMemcpyDeviceToHost));
    out->iterations = o.iterations;
    out->converged = o.converged;
    out->cost0 = o.cost0;
    out->cost = o.cost;
    out->max_step = o.max_step;
    out->cg_iterations = o.cg_iterations;
    return NDT_OK;
}

ndt_status ndt_pgo_get_poses(ndt_pgo* g, double* poses16, int cap, int* n_out) {
    if (!g) return NDT_EINVAL;
    const int n = ndt_pgo_size(g);
    if (n_out) *n_out = n;
    if (cap < 0 || (cap && !poses16)) return fail(g->c, NDT_EINVAL, "bad output arguments");
    for (int k = 0; k < std::min(n, cap); ++k) {
        const double* P = g->X.data() + 12 * (size_t)k;
        double* m = poses16 + 16 * (size_t)k;
        for (int r = 0; r < 3; ++r) {
            for (int col = 0; col < 3; ++col) m[4 * col + r] = P[3 * r + col];
            m[12 + r] = P[9 + r];
            m[4 * r + 3] = 0.0;
        }
        m[15] = 1.0;
    }
    return NDT_OK;
}

ndt_status ndt_pgo_get_weights(ndt_pgo* g, double* w, int cap, int* n_out) {
    if (!g) return NDT_EINVAL;
    const int n = (int)g->weights.size();
    if (n_out) *n_out = n;
    if (cap < 0 || (cap && !w)) return fail(g->c, NDT_EINVAL, "bad output arguments");
    std::copy(g->weights.begin(), g->weights.begin() + std::min(n, cap), w);
    return NDT_OK;
}

ndt_status ndt_pgo_get_position_weights(ndt_pgo* g, double* w, int cap, int* n_out) {
    if (!g) return NDT_EINVAL;
    const int n = (int)g->pweights.size();
    if (n_out) *n_out = n;
    if (cap < 0 || (cap && !w)) return fail(g->c, NDT_EINVAL, "bad output arguments");
    std::copy(g->pweights.begin(), g->pweights.begin() + std::min(n, cap), w);
    return NDT_OK;
}

ndt_status ndt_pgo_history(ndt_pgo* g, ndt_pgo_record* out, int cap, int* n_out) {
    if (!g) return NDT_EINVAL;
    const int n = (int)g->hist.size();
    if (n_out) *n_out = n;
    if (cap < 0 || (cap && !out)) return fail(g->c, NDT_EINVAL, "bad output arguments");
    std::copy(g->hist.begin(), g->hist.begin() + std::min(n, cap), out);
    return NDT_OK;
}

}  // extern "C"
