// posegraph_direct.hip — the direct loop-space solve of the pose graph's Gauss-Newton step (DESIGN.md §4 "Pose-graph
// kernel", direct solve), the second linear solver beside k_pgo_optimize's conjugate gradients.
//
// The step solves (I + B^T B) y = g.  By Woodbury  (I + B^T B)^-1 = I - B^T S^-1 B  with  S = I_d + B B^T, d = 6 m + 3 np,
// dense, symmetric and with every eigenvalue >= 1.  S is built from the table C_k = sum_{t <= k} P_t P_t^T
// (ndt_pgo_schur.h), factorised by a blocked right-looking Cholesky, and one outer iteration is a fixed sequence of
// launches on one stream:
//     k_pgo_direct_step   one workgroup: (the step of the previous iteration: f = B^T-gather of z, y = g - P^T suffix(f),
//                         d = G L P y, the retraction, the record;) then the linearisation at the new estimate: residuals,
//                         weights, Kw per factor, g, u = L P g, b = Kw (u_j - u_i), the table C; the status block
//     k_pgo_schur         the lower triangle of S, 16 x 16 factor pairs per workgroup, one pair per thread
//     k_pgo_chol_diag     per tile column: the diagonal tile factored in LDS by one workgroup,
//     k_pgo_chol_panel    the tiles below it solved one per workgroup (b, carried as row dp, is one more: the forward solve),
//     k_pgo_chol_trail    the trailing lower-triangle tiles (and b's) updated one per workgroup
//     k_pgo_chol_back     one workgroup going up tile by tile: z = L^-T (L^-1 b), left in row dp
// The host reads the status block once per outer iteration and decides whether to enqueue the next.
//
// Determinism: workgroups depend on each other through kernel boundaries only; every sum has a fixed order (the scans
// are scan6's, a tile's inner products run over k ascending, the trailing update adds one panel per launch in column
// order); there are no floating-point atomics and no wait loops.
#include "ndt_kernels.h"
#include "ndt_pgo_dev.h"
#include "ndt_pgo_schur.h"

namespace ndt {
namespace {

constexpr int T = kPgoDirectTile;
constexpr int kCholBlock = 256;

// P_k P_k^T, 6 x 6 row-major
__device__ inline void ppt(const PgoGraph& g, const PgoArgs& a, int k, double* o) {
    double P[6][6];  // P[c] = column c of P_k
    for (int c = 0; c < 6; ++c) {
        double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        e[c] = 1.0;
        apply_p(g, a, k, e, P[c]);
    }
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) {
            double acc = 0.0;
            for (int t = 0; t < 6; ++t) acc = acc + P[t][r] * P[t][c];
            o[6 * r + c] = acc;
            o[6 * c + r] = acc;
        }
}

// What the next launches read: g (into g.r), u = L P g (into g.z), b (row dp of S), the table C, S's padding.
__device__ void linearise(const PgoGraph& g, const PgoArgs& a, const PgoDirect& dg, PgoLds& s) {
    const int n = g.n;
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
            for (int i = 0; i < 6; ++i) g.r[6 * (size_t)k + i] = o[i];
        });
    if (dg.d == 0) return;
    scan6<false>(
        n, g.tmp, s, [&](int k, double* v) { apply_p(g, a, k, g.r + 6 * (size_t)k, v); },
        [](int, const double* v, double* o) {
            for (int i = 0; i < 6; ++i) o[i] = v[i];
        },
        [&](int k, const double* o) {
            for (int i = 0; i < 6; ++i) g.z[6 * (size_t)k + i] = o[i];
        });
    double* b = dg.S + (size_t)dg.dp * dg.dp;
    for (int q = threadIdx.x; q < g.m; q += kPgoBlock) {
        const double* ui = g.z + 6 * (size_t)g.li[q];
        const double* uj = g.z + 6 * (size_t)g.lj[q];
        double du[6];
        for (int i = 0; i < 6; ++i) du[i] = uj[i] - ui[i];
        for (int r = 0; r < 6; ++r) {
            const double* kr = dg.kw + 36 * (size_t)q + 6 * r;
            double acc = 0.0;
            for (int c = 0; c < 6; ++c) acc = acc + kr[c] * du[c];
            b[6 * q + r] = acc;
        }
    }
    // a position factor's Kw = diag(sqrt(w iv)) [-hat(t_k), I]
    for (int q = threadIdx.x; q < g.np; q += kPgoBlock) {
        const int k = g.poff[g.n + 1 + q];
        const double* t = g.X + 12 * (size_t)k + 9;
        const double* u = g.z + 6 * (size_t)k;
        const double* work = g.pf + 7 * ((size_t)g.np + q);
        double H[9], ku[3];
        hat3(t, H);
        cross3(t, u, ku);
        const int row = 6 * g.m + 3 * q;
        for (int i = 0; i < 3; ++i) {
            const double sw = sqrt(work[i]);
            double* kr = dg.kw + 6 * (size_t)(row + i);
            for (int c = 0; c < 3; ++c) {
                kr[c] = sw * -H[3 * i + c];
                kr[3 + c] = c == i ? sw : 0.0;
            }
            b[row + i] = sw * (u[3 + i] - ku[i]);
        }
    }
    // the padding of S up to whole tiles: identity rows, and zeros in b
    for (int e = threadIdx.x; e < (dg.dp - dg.d) * dg.dp; e += kPgoBlock) {
        const int r = dg.d + e / dg.dp, c = e % dg.dp;
        dg.S[(size_t)r * dg.dp + c] = r == c ? 1.0 : 0.0;
    }
    for (int c = dg.d + threadIdx.x; c < dg.dp; c += kPgoBlock) b[c] = 0.0;
    // C: P_t P_t^T per node, then six scans of six values in scan6's order
    for (int k = threadIdx.x; k < n; k += kPgoBlock) {
        double o[36];
        ppt(g, a, k, o);
        for (int i = 0; i < 36; ++i) dg.C[36 * (size_t)k + i] = o[i];
    }
    __syncthreads();
    for (int r = 0; r < 6; ++r)
        scan6<false>(
            n, g.tmp, s,
            [&](int k, double* v) {
                for (int i = 0; i < 6; ++i) v[i] = dg.C[36 * (size_t)k + 6 * r + i];
            },
            [](int, const double* v, double* o) {
                for (int i = 0; i < 6; ++i) o[i] = v[i];
            },
            [&](int k, const double* o) {
                for (int i = 0; i < 6; ++i) dg.C[36 * (size_t)k + 6 * r + i] = o[i];
            });
}

}  // namespace

// first: the linearisation at the input alone; otherwise the step from row dp's z, then the linearisation.
__global__ __launch_bounds__(kPgoBlock) void k_pgo_direct_step(PgoGraph g, PgoArgs a, PgoDirect dg, int first) {
    __shared__ PgoLds s;
    const int n = g.n;
    if (threadIdx.x == 0) s.bad = 0x7fffffff;
    const PgoDirectState in = *dg.st;
    __syncthreads();
    int it = in.iterations, converged = 0, status = kPgoOk;
    double cost0 = in.cost0, cost = in.cost, step = in.max_step;
    if (!first) {
        if (in.pivot_bad) {
            status = kPgoNotFinite;  // no step was taken from this estimate: X is the one before it
        } else {
            // f = sum_{a contains k} s Kw_a^T z_a: per factor here, per node in the gathers of the suffix sum
            const double* z = dg.S + (size_t)dg.dp * dg.dp;
            for (int q = threadIdx.x; q < g.m; q += kPgoBlock) {
                const double* K = dg.kw + 36 * (size_t)q;
                for (int c = 0; c < 6; ++c) {
                    double acc = 0.0;
                    for (int r = 0; r < 6; ++r) acc = acc + K[6 * r + c] * z[6 * q + r];
                    g.dl[6 * (size_t)q + c] = acc;
                }
            }
            for (int q = threadIdx.x; q < g.np; q += kPgoBlock) {
                double* work = g.pf + 7 * ((size_t)g.np + q);
                for (int i = 0; i < 3; ++i) work[3 + i] = sqrt(work[i]) * z[6 * g.m + 3 * q + i];
            }
            __syncthreads();
            // y = g - P^T (suffix sum of f)
            scan6<true>(
                n, g.tmp, s,
                [&](int k, double* v) {
                    gather_node(g, k, g.dl, v);
                    gather_positions<false>(g, k, v);
                },
                [&](int k, const double* v, double* o) {
                    apply_pt(g, a, k, v, o);
                    for (int i = 0; i < 6; ++i) o[i] = g.r[6 * (size_t)k + i] - o[i];
                },
                [&](int k, const double* o) {
                    for (int i = 0; i < 6; ++i) g.y[6 * (size_t)k + i] = o[i];
                });
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
                g.hist[it].cg_iterations = 0;
            }
            ++it;
            if (!isfinite(step)) {  // (block_max's barriers: Xprev is complete)
                status = kPgoNotFinite;
                for (int i = threadIdx.x; i < 12 * n; i += kPgoBlock) g.X[i] = g.Xprev[i];
            }
            converged = step < a.step_eps;
        }
    }
    int done = status != kPgoOk;
    if (!done) {
        cost = evaluate<true>(g, a, s, dg.kw);
        const int bad = s.bad;  // (block_sum's barriers order the atomicMin before this read)
        if (bad != 0x7fffffff) {
            status = kPgoNearPi;
            if (threadIdx.x == 0) dg.st->bad = bad;
        } else if (!isfinite(cost)) {
            status = kPgoNotFinite;
        }
        if (status != kPgoOk) {
            // the estimate before the step that led here (the input itself when no step was taken)
            if (it > 0)
                for (int i = threadIdx.x; i < 12 * n; i += kPgoBlock) g.X[i] = g.Xprev[i];
            done = 1;
        } else {
            if (it == 0) cost0 = cost;
            done = converged || it >= a.max_iter;
            if (!done) linearise(g, a, dg, s);
        }
    }
    if (threadIdx.x == 0) {
        dg.st->status = status;
        dg.st->iterations = it;
        dg.st->converged = converged;
        dg.st->done = done;
        dg.st->cost0 = cost0;
        dg.st->cost = cost;
        dg.st->max_step = step;
    }
}

// The lower triangle of S (rows < d): thread (ty, tx) of workgroup (bx, by) builds the block of the factor pair
// (16 by + ty, 16 bx + tx), b <= a.  A diagonal pair gets the identity and is written whole.
__global__ __launch_bounds__(256) void k_pgo_schur(PgoGraph g, PgoDirect dg) {
    if (blockIdx.x > blockIdx.y) return;
    const int fa = 16 * blockIdx.y + (threadIdx.x >> 4), fb = 16 * blockIdx.x + (threadIdx.x & 15);
    const int nf = g.m + g.np;
    if (fa >= nf || fb > fa) return;
    const int* pnode = g.poff + g.n + 1;
    const PgoFactorRef a = pgo_factor_ref(fa, g.m, g.li, g.lj, pnode), b = pgo_factor_ref(fb, g.m, g.li, g.lj, pnode);
    double* out = dg.S + (size_t)a.row * dg.dp + b.row;
    pgo_schur_block(dg.C, dg.kw, a, b, out, (size_t)dg.dp);
    if (fa == fb)
        for (int r = 0; r < a.nr; ++r) out[(size_t)r * dg.dp + r] = 1.0 + out[(size_t)r * dg.dp + r];
}

// Tile (kt, kt) <- its Cholesky factor (lower; the upper half is not read anywhere).
__global__ __launch_bounds__(kCholBlock) void k_pgo_chol_diag(PgoDirect dg, int kt) {
    __shared__ double A[T][T + 1];
    const size_t ld = dg.dp;
    double* tile = dg.S + (size_t)kt * T * ld + (size_t)kt * T;
    for (int e = threadIdx.x; e < T * T; e += kCholBlock) {
        const int r = e / T, c = e % T;
        A[r][c] = c <= r ? tile[r * ld + c] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < T; ++j) {
        if (threadIdx.x == 0) {
            const double p = A[j][j];
            if (!(isfinite(p) && p >= kPgoPivotMin)) dg.st->pivot_bad = 1;
            A[j][j] = sqrt(p);
        }
        __syncthreads();
        if (threadIdx.x > j && threadIdx.x < T) A[threadIdx.x][j] = A[threadIdx.x][j] / A[j][j];
        __syncthreads();
        for (int e = threadIdx.x; e < T * T; e += kCholBlock) {
            const int r = e / T, c = e % T;
            if (c > j && c <= r) A[r][c] = A[r][c] - A[r][j] * A[c][j];
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < T * T; e += kCholBlock) {
        const int r = e / T, c = e % T;
        if (c <= r) tile[r * ld + c] = A[r][c];
    }
}

// Workgroup w: tile (kt + 1 + w, kt) <- tile L_kk^-T; the last workgroup does b's part (one row), which is the forward solve.
__global__ __launch_bounds__(kCholBlock) void k_pgo_chol_panel(PgoDirect dg, int kt) {
    __shared__ double L[T][T + 1], A[T][T + 1];
    const size_t ld = dg.dp;
    const int nt = dg.dp / T;
    const bool brow = (int)blockIdx.x == nt - kt - 1;
    const int rows = brow ? 1 : T;
    const double* diag = dg.S + (size_t)kt * T * ld + (size_t)kt * T;
    double* tile = dg.S + (brow ? (size_t)dg.dp : (size_t)(kt + 1 + blockIdx.x) * T) * ld + (size_t)kt * T;
    for (int e = threadIdx.x; e < T * T; e += kCholBlock) {
        const int r = e / T, c = e % T;
        L[r][c] = c <= r ? diag[r * ld + c] : 0.0;
        A[r][c] = r < rows ? tile[r * ld + c] : 0.0;
    }
    __syncthreads();
    // x L^T = a per row, column by column: x_c = a_c / L_cc, then a_c' -= x_c L_c'c for c' > c
    for (int c = 0; c < T; ++c) {
        if (threadIdx.x < T) A[threadIdx.x][c] = A[threadIdx.x][c] / L[c][c];
        __syncthreads();
        for (int e = threadIdx.x; e < T * T; e += kCholBlock) {
            const int r = e / T, c2 = e % T;
            if (c2 > c) A[r][c2] = A[r][c2] - A[r][c] * L[c2][c];
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < rows * T; e += kCholBlock) {
        const int r = e / T, c = e % T;
        tile[r * ld + c] = A[r][c];
    }
}

// Workgroup (x, y), x <= y: tile (kt + 1 + y, kt + 1 + x) -= A_(y, kt) A_(x, kt)^T; y == the last: b's part.
__global__ __launch_bounds__(kCholBlock) void k_pgo_chol_trail(PgoDirect dg, int kt) {
    if (blockIdx.x > blockIdx.y) return;
    __shared__ double Ai[T][T + 1], Aj[T][T + 1];
    const size_t ld = dg.dp;
    const int rem = dg.dp / T - kt - 1;
    const bool brow = (int)blockIdx.y == rem;
    if (brow && (int)blockIdx.x == rem) return;
    const int rows = brow ? 1 : T;
    const size_t row0 = brow ? (size_t)dg.dp : (size_t)(kt + 1 + blockIdx.y) * T;
    const size_t col0 = (size_t)(kt + 1 + blockIdx.x) * T;
    const double* pi = dg.S + row0 * ld + (size_t)kt * T;
    const double* pj = dg.S + col0 * ld + (size_t)kt * T;
    for (int e = threadIdx.x; e < T * T; e += kCholBlock) {
        const int r = e / T, c = e % T;
        Ai[r][c] = r < rows ? pi[r * ld + c] : 0.0;
        Aj[r][c] = pj[r * ld + c];
    }
    __syncthreads();
    double* out = dg.S + row0 * ld + col0;
    for (int e = threadIdx.x; e < rows * T; e += kCholBlock) {
        const int r = e / T, c = e % T;
        double acc = 0.0;
        for (int k = 0; k < T; ++k) acc = acc + Ai[r][k] * Aj[c][k];
        out[r * ld + c] = out[r * ld + c] - acc;
    }
}

// z = L^-T y, y = row dp (the forward solve), going up tile by tile; z replaces y.
__global__ __launch_bounds__(kCholBlock) void k_pgo_chol_back(PgoDirect dg) {
    __shared__ double L[T][T + 1], part[kCholBlock / T][T], rhs[T];
    const size_t ld = dg.dp;
    const int nt = dg.dp / T;
    double* z = dg.S + (size_t)dg.dp * ld;
    const int c = threadIdx.x % T, grp = threadIdx.x / T;
    for (int kt = nt - 1; kt >= 0; --kt) {
        // sum over the rows below this tile of L[r][col] z[r]: each thread its rows in order, then the groups in order
        double acc = 0.0;
        for (int r = (kt + 1) * T + grp; r < dg.dp; r += kCholBlock / T) acc = acc + dg.S[(size_t)r * ld + (size_t)kt * T + c] * z[r];
        part[grp][c] = acc;
        const double* diag = dg.S + (size_t)kt * T * ld + (size_t)kt * T;
        for (int e = threadIdx.x; e < T * T; e += kCholBlock) {
            const int r = e / T, cc = e % T;
            L[r][cc] = cc <= r ? diag[r * ld + cc] : 0.0;
        }
        __syncthreads();
        if (threadIdx.x < T) {
            double t = part[0][c];
            for (int k = 1; k < kCholBlock / T; ++k) t = t + part[k][c];
            rhs[c] = z[kt * T + c] - t;
        }
        __syncthreads();
        for (int j = T - 1; j >= 0; --j) {
            if ((int)threadIdx.x == j) rhs[j] = rhs[j] / L[j][j];
            __syncthreads();
            if ((int)threadIdx.x < j) rhs[threadIdx.x] = rhs[threadIdx.x] - L[j][threadIdx.x] * rhs[j];
            __syncthreads();
        }
        if (threadIdx.x < T) z[kt * T + c] = rhs[c];
        __syncthreads();
    }
}

}  // namespace ndt
