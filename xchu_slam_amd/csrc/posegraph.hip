// posegraph.hip — k_pgo_optimize: a whole robust SE(3) pose-graph optimisation in one launch of one workgroup
// (DESIGN.md §4 "Pose-graph kernel").  Linearisation, robust weights, the linear solve, the retraction, the convergence
// test and the per-iteration record all run here; the host reads the result once.
//
// Each outer iteration is one iteratively reweighted Gauss-Newton step.  Its normal equations are solved by conjugate
// gradients preconditioned with the exact solve of the chain part (prior + odometry), written as plain CG on the
// variable y = Ac d:  (I + B^T B) y = -rc - B^T rl,  B = W^1/2 Al Ac^-1.
// Ac (the chain's whitened Jacobian) is square and block lower-bidiagonal, and because de/ddi is an adjoint its inverse
// is   Ac^-1 = G L P,   P_k = Ad(X_k) Jr(e_k) diag(sigma_k),  L = prefix sum over the nodes,  G_k = Ad(X_k^-1),
// and a loop edge's row of Al Ac^-1 is  K_e (E_j - E_i) L P  with  K_e = S Jr^-1(e) Ad(X_j^-1): in the world frame a
// loop sees the difference of two prefix sums.  One product with I + B^T B is therefore a prefix sum, one 6 x 6 product
// per loop edge (N_e = w K^T K), a per-node gather over the host-built edge lists, a suffix sum and P^T.
// A position factor on node k (residual t_k - z, Jacobian [0 R_k]) sees one prefix sum: its row of Al Ac^-1 is
// S^-1/2 K_k E_k L P with K_k = [-hat(t_k), I], so K u = u_v - t_k x u_w and K^T c = [t_k x c; c].  It adds
// w K^T (iv . (K z_k)) to node k's gather in the product and w K^T (iv . r) in the right-hand side (iv = 1 / var), both
// formed in the gather itself from three stored doubles; a node's between edges come first, then its position factors
// in insertion order.
//
// The reductions, the scan, P, P^T, the gathers and the linearisation are ndt_pgo_dev.h's, shared with the direct solve
// (posegraph_direct.hip).
//
// Determinism: every sum runs in a fixed order (per-thread runs, wave shuffles, then the waves in order); there are no
// floating-point atomics.  Nothing here waits on another workgroup, so there is no wait loop.
#include "ndt_kernels.h"
#include "ndt_pgo_dev.h"

namespace ndt {
namespace {

// hp = (I + B^T B) p; returns p . hp
__device__ double apply_h(const PgoGraph& g, const PgoArgs& a, PgoLds& s) {
    scan6<false>(
        g.n, g.tmp, s, [&](int k, double* v) { apply_p(g, a, k, g.p + 6 * (size_t)k, v); },
        [](int, const double* v, double* o) {
            for (int i = 0; i < 6; ++i) o[i] = v[i];
        },
        [&](int k, const double* o) {
            for (int i = 0; i < 6; ++i) g.z[6 * (size_t)k + i] = o[i];
        });
    for (int q = threadIdx.x; q < g.m; q += kPgoBlock) {
        const double* zi = g.z + 6 * (size_t)g.li[q];
        const double* zj = g.z + 6 * (size_t)g.lj[q];
        const double* N = g.N + 36 * (size_t)q;
        double d[6], t[6];
        for (int i = 0; i < 6; ++i) d[i] = zj[i] - zi[i];
        for (int r = 0; r < 6; ++r) {
            t[r] = 0.0;
            for (int c = 0; c < 6; ++c) t[r] = t[r] + N[6 * r + c] * d[c];
        }
        for (int r = 0; r < 6; ++r) g.dl[6 * (size_t)q + r] = t[r];
    }
    __syncthreads();
    double dot = 0.0;  // this thread's nodes, in its run's order
    scan6<true>(
        g.n, g.tmp, s,
        [&](int k, double* v) {
            gather_node(g, k, g.dl, v);
            gather_positions<true>(g, k, v);
        },
        [&](int k, const double* v, double* o) {
            apply_pt(g, a, k, v, o);
            for (int i = 0; i < 6; ++i) {
                const double pk = g.p[6 * (size_t)k + i];
                o[i] = pk + o[i];
                dot = dot + pk * o[i];
            }
        },
        [&](int k, const double* o) {
            for (int i = 0; i < 6; ++i) g.hp[6 * (size_t)k + i] = o[i];
        });
    return block_sum(dot, s);
}

}  // namespace

__global__ __launch_bounds__(kPgoBlock) void k_pgo_optimize(PgoGraph g, PgoArgs a) {
    __shared__ PgoLds s;
    const int n = g.n, n6 = 6 * g.n;
    if (threadIdx.x == 0) s.bad = 0x7fffffff;
    __syncthreads();
    int it = 0, converged = 0, cg_total = 0, status = kPgoOk;
    double cost0 = 0.0, cost = 0.0, step = 0.0;
    for (;;) {
        cost = evaluate<false>(g, a, s);
        const int bad = s.bad;  // (block_sum's barriers order the atomicMin before this read)
        if (bad != 0x7fffffff) {
            status = kPgoNearPi;
            if (threadIdx.x == 0) g.out->bad = bad;
        } else if (!isfinite(cost)) {
            status = kPgoNotFinite;
        }
        if (status != kPgoOk) {
            // the estimate before the step that led here (the input itself when no step was taken)
            if (it > 0)
                for (int i = threadIdx.x; i < 12 * n; i += kPgoBlock) g.X[i] = g.Xprev[i];
            break;
        }
        if (it == 0) cost0 = cost;
        if (converged || it >= a.max_iter) break;

        // right-hand side  -rc - B^T rl  into r, p; y = 0
        scan6<true>(
            n, g.tmp, s,
            [&](int k, double* v) {
                gather_node(g, k, g.bv, v);
                gather_positions<false>(g, k, v);
            },
            [&](int k, const double* v, double* o) {
                apply_pt(g, a, k, v, o);
                for (int i = 0; i < 6; ++i) o[i] = -g.rc[6 * (size_t)k + i] - o[i];
            },
            [&](int k, const double* o) {
                for (int i = 0; i < 6; ++i) {
                    g.r[6 * (size_t)k + i] = o[i];
                    g.p[6 * (size_t)k + i] = o[i];
                    g.y[6 * (size_t)k + i] = 0.0;
                }
            });
        double part = 0.0;
        for (int i = threadIdx.x; i < n6; i += kPgoBlock) part = part + g.r[i] * g.r[i];
        double rr = block_sum(part, s);
        const double stop = a.cg_rtol * a.cg_rtol * rr;
        int cg = 0;
        while (cg < a.cg_max_iter && rr > stop && rr > 0.0) {
            const double alpha = rr / apply_h(g, a, s);
            part = 0.0;
            for (int i = threadIdx.x; i < n6; i += kPgoBlock) {
                g.y[i] = g.y[i] + alpha * g.p[i];
                const double r = g.r[i] - alpha * g.hp[i];
                g.r[i] = r;
                part = part + r * r;
            }
            const double rn = block_sum(part, s);
            const double beta = rn / rr;
            for (int i = threadIdx.x; i < n6; i += kPgoBlock) g.p[i] = g.r[i] + beta * g.p[i];
            rr = rn;
            ++cg;
            __syncthreads();
        }
        cg_total += cg;

        // d = G L P y, then X <- X Exp(d)
        scan6<false>(
            n, g.tmp, s, [&](int k, double* v) { apply_p(g, a, k, g.y + 6 * (size_t)k, v); },
            [&](int k, const double* v, double* o) { ad_inv_vec(g.X + 12 * (size_t)k, v, o); },
            [&](int k, const double* o) {
                for (int i = 0; i < 6; ++i) g.hp[6 * (size_t)k + i] = o[i];
            });
        double mx = 0.0;
        for (int k = threadIdx.x; k < n; k += kPgoBlock) {
            double* Xk = g.X + 12 * (size_t)k;
            const double* d = g.hp + 6 * (size_t)k;
            double D[12], Xn[12];
            for (int i = 0; i < 6; ++i) mx = fmax(mx, isfinite(d[i]) ? fabs(d[i]) : INFINITY);  // fmax alone drops a NaN
            pgo_exp(d, D);
            pose_mul(Xk, D, Xn);
            for (int i = 0; i < 12; ++i) {
                g.Xprev[12 * (size_t)k + i] = Xk[i];
                Xk[i] = Xn[i];
            }
        }
        step = block_max(mx, s);
        if (threadIdx.x == 0) {
            g.hist[it].cost = cost;
            g.hist[it].max_step = step;
            g.hist[it].cg_iterations = cg;
        }
        ++it;
        if (!isfinite(step)) {  // (block_max's barriers: Xprev is complete)
            status = kPgoNotFinite;
            for (int i = threadIdx.x; i < 12 * n; i += kPgoBlock) g.X[i] = g.Xprev[i];
            break;
        }
        converged = step < a.step_eps;
    }
    if (threadIdx.x == 0) {
        g.out->status = status;
        g.out->iterations = it;
        g.out->converged = converged;
        g.out->cg_iterations = cg_total;
        g.out->cost0 = cost0;
        g.out->cost = cost;
        g.out->max_step = step;
    }
}

}  // namespace ndt
