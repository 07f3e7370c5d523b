// ndt_pgo_dev.h — the device parts the pose-graph kernels share (posegraph.hip: k_pgo_optimize, conjugate gradients;
// posegraph_direct.hip: the direct loop-space solve): the workgroup reductions, the 6-vector scan over the nodes, P and
// P^T, the per-node gathers and the linearisation.  Everything here runs in one workgroup of kPgoBlock threads.
#pragma once
#include "ndt_pgo.h"

namespace ndt {

struct PgoLds {
    double wave[kPgoWaves][6];
    double bcast;
    int bad;
};

__device__ inline int chunk_of(int n) { return (n + kPgoBlock - 1) / kPgoBlock; }

// Sum (MAX: maximum) over the workgroup in a fixed order; every thread gets the result.
template <bool MAX> __device__ inline double block_reduce(double v, PgoLds& s) {
    auto op = [](double x, double y) { return MAX ? fmax(x, y) : x + y; };
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_down(v, d, 64));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s.wave[wv][0] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s.wave[0][0];
        for (int k = 1; k < kPgoWaves; ++k) t = op(t, s.wave[k][0]);
        s.bcast = t;
    }
    __syncthreads();
    const double out = s.bcast;
    __syncthreads();  // s is free for the next reduction or scan
    return out;
}
__device__ inline double block_sum(double v, PgoLds& s) { return block_reduce<false>(v, s); }
__device__ inline double block_max(double v, PgoLds& s) { return block_reduce<true>(v, s); }

// Inclusive prefix (REV: suffix) sums of the n 6-vectors load(k) in node order; store(k, map(k, sum)) receives each.
// A thread owns a run of consecutive nodes: it sums its run (the running sums parked in tmp), the runs' totals are
// scanned over the workgroup (wave shuffles, then the waves in order), and each running sum gets its run's offset.
// Both sweeps take the run kScanBatch nodes at a time, all of a batch's loads and arithmetic ahead of its stores, so the
// memory round trips of a batch overlap; the order of every sum is that of the node order whatever the batch.
// Ends with a barrier: what store wrote is visible to the whole workgroup.
constexpr int kScanBatch = 4;

template <bool REV, typename Load, typename Map, typename Store>
__device__ inline void scan6(int n, double* tmp, PgoLds& s, Load load, Map map, Store store) {
    const int c = chunk_of(n);
    const int lo = min(n, (int)threadIdx.x * c), hi = min(n, lo + c);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k0 = lo; k0 < hi; k0 += kScanBatch) {
        double v[kScanBatch][6];
#pragma unroll
        for (int u = 0; u < kScanBatch; ++u)
            if (k0 + u < hi) load(REV ? n - 1 - (k0 + u) : k0 + u, v[u]);
#pragma unroll
        for (int u = 0; u < kScanBatch; ++u)
            if (k0 + u < hi) {
                const int node = REV ? n - 1 - (k0 + u) : k0 + u;
                for (int a = 0; a < 6; ++a) {
                    acc[a] = acc[a] + v[u][a];
                    tmp[6 * (size_t)node + a] = acc[a];
                }
            }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double off[6];
    for (int a = 0; a < 6; ++a) {
        double inc = acc[a];
        for (int d = 1; d < 64; d <<= 1) {
            const double up = __shfl_up(inc, d, 64);
            if (lane >= d) inc = up + inc;
        }
        if (lane == 63) s.wave[wv][a] = inc;
        const double prev = __shfl_up(inc, 1, 64);
        off[a] = lane ? prev : 0.0;
    }
    __syncthreads();
    for (int a = 0; a < 6; ++a) {
        double base = 0.0;
        for (int k = 0; k < wv; ++k) base = base + s.wave[k][a];
        off[a] = base + off[a];
    }
    for (int k0 = lo; k0 < hi; k0 += kScanBatch) {
        double o[kScanBatch][6];
#pragma unroll
        for (int u = 0; u < kScanBatch; ++u)
            if (k0 + u < hi) {
                const int node = REV ? n - 1 - (k0 + u) : k0 + u;
                double v[6];
                for (int a = 0; a < 6; ++a) v[a] = off[a] + tmp[6 * (size_t)node + a];
                map(node, v, o[u]);
            }
#pragma unroll
        for (int u = 0; u < kScanBatch; ++u)
            if (k0 + u < hi) store(REV ? n - 1 - (k0 + u) : k0 + u, o[u]);
    }
    __syncthreads();
}

// o = P_k v = Ad(X_k) Jr(e_k) (sigma . v)
__device__ inline void apply_p(const PgoGraph& g, const PgoArgs& a, int k, const double* v, double* o) {
    const double* sig = k ? a.sig_odom : a.sig_prior;
    const double* J = g.Jc + 18 * (size_t)k;
    double sv[6], t[6], q[3];
    for (int i = 0; i < 6; ++i) sv[i] = sig[i] * v[i];
    m3_vec(J, sv, t);
    m3_vec(J, sv + 3, t + 3);
    m3_vec(J + 9, sv, q);
    for (int i = 0; i < 3; ++i) t[3 + i] = q[i] + t[3 + i];
    ad_vec(g.X + 12 * (size_t)k, t, o);
}

// o = P_k^T v = sigma . (Jr(e_k)^T Ad(X_k)^T v)
__device__ inline void apply_pt(const PgoGraph& g, const PgoArgs& a, int k, const double* v, double* o) {
    const double* sig = k ? a.sig_odom : a.sig_prior;
    const double* J = g.Jc + 18 * (size_t)k;
    double t[6], q[3];
    ad_t_vec(g.X + 12 * (size_t)k, v, t);
    m3_tvec(J, t, o);
    m3_tvec(J + 9, t + 3, q);
    for (int i = 0; i < 3; ++i) o[i] = o[i] + q[i];
    m3_tvec(J, t + 3, o + 3);
    for (int i = 0; i < 6; ++i) o[i] = sig[i] * o[i];
}

// The sum over node k's loop edges of +-src[edge] (+ where the node is the edge's j)
__device__ inline void gather_node(const PgoGraph& g, int k, const double* src, double* f) {
    for (int a = 0; a < 6; ++a) f[a] = 0.0;
    for (int q = g.off[k]; q < g.off[k + 1]; ++q) {
        const int en = g.ent[q];
        const double* d = src + 6 * (size_t)(en >> 1);
        if (en & 1)
            for (int a = 0; a < 6; ++a) f[a] = f[a] + d[a];
        else
            for (int a = 0; a < 6; ++a) f[a] = f[a] - d[a];
    }
}

// Adds node k's position factors to the gather f: w K^T (iv . (K z_k)) (OP: the matrix-vector step, after g.z is
// complete), else w K^T (iv . r), in insertion order.  t_k is read from g.X, which does not move during CG.
template <bool OP> __device__ inline void gather_positions(const PgoGraph& g, int k, double* f) {
    const int lo = g.poff[k], hi = g.poff[k + 1];
    if (lo == hi) return;
    const double* t = g.X + 12 * (size_t)k + 9;
    double ku[3];
    if (OP) {
        const double* u = g.z + 6 * (size_t)k;
        cross3(t, u, ku);
        for (int i = 0; i < 3; ++i) ku[i] = u[3 + i] - ku[i];
    }
    const double* work = g.pf + 7 * (size_t)g.np;
    for (int q = lo; q < hi; ++q) {
        double c[3], x[3];
        for (int i = 0; i < 3; ++i) c[i] = OP ? work[7 * (size_t)q + i] * ku[i] : work[7 * (size_t)q + 3 + i];
        cross3(t, c, x);
        for (int i = 0; i < 3; ++i) {
            f[i] = f[i] + x[i];
            f[3 + i] = f[3 + i] + c[i];
        }
    }
}

// Residuals, robust weights and the linearisation at the current estimate; returns the total robust cost, or sets
// s.bad to the lowest factor whose residual rotation is within kPgoPiMargin of pi.  KW (the direct solve): also stores
// each between factor's Kw = diag(sqrt(w iv)) M, 6 x 6 row-major, at kw + 36 q.
template <bool KW> __device__ inline double evaluate(const PgoGraph& g, const PgoArgs& a, PgoLds& s, double* kw = nullptr) {
    double cost = 0.0;
    for (int k = threadIdx.x; k < g.n; k += kPgoBlock) {
        double rel[12], E[12], e[6];
        const double* Xk = g.X + 12 * (size_t)k;
        if (k) {
            pose_inv_mul(Xk - 12, Xk, rel);
            pose_inv_mul(g.Zc + 12 * (size_t)k, rel, E);
        } else {
            pose_inv_mul(g.Zc, Xk, E);
        }
        if (!pgo_log(E, e)) {
            atomicMin(&s.bad, k);
            continue;
        }
        const double* sig = k ? a.sig_odom : a.sig_prior;
        double c = 0.0;
        for (int i = 0; i < 6; ++i) {
            const double r = e[i] / sig[i];
            g.rc[6 * (size_t)k + i] = r;
            c = c + r * r;
        }
        cost = cost + 0.5 * c;
        pgo_jr(e, g.Jc + 18 * (size_t)k, g.Jc + 18 * (size_t)k + 9);
    }
    for (int q = threadIdx.x; q < g.m; q += kPgoBlock) {
        double rel[12], E[12], e[6];
        const double* Xi = g.X + 12 * (size_t)g.li[q];
        const double* Xj = g.X + 12 * (size_t)g.lj[q];
        pose_inv_mul(Xi, Xj, rel);
        pose_inv_mul(g.Zl + 12 * (size_t)q, rel, E);
        if (!pgo_log(E, e)) {
            atomicMin(&s.bad, g.n + q);
            continue;
        }
        const double* var = g.lvar + 6 * (size_t)q;
        double s2 = 0.0, iv[6];
        for (int i = 0; i < 6; ++i) {
            iv[i] = 1.0 / var[i];
            s2 = s2 + e[i] * e[i] * iv[i];
        }
        const double rk = g.lk[q];
        double w = 1.0;
        if (rk > 0.0) {
            const double k2 = rk * rk;
            w = k2 / (k2 + s2);
            cost = cost + 0.5 * k2 * log1p(s2 / k2);
        } else {
            cost = cost + 0.5 * s2;
        }
        g.w[q] = w;
        // M = Jr^-1(e) Ad(Xj^-1) = [[Ji Rt, 0], [Q2 Rt + Ji G, Ji Rt]],  Rt = Rj^T,  G = -Rj^T hat(tj)
        double Ji[9], Q2[9], T[9], G[9], UL[9], LL[9], t1[9];
        pgo_jr_inv(e, Ji, Q2);
        hat3(Xj + 9, T);
        m3_tmul(Xj, T, G);
        for (int i = 0; i < 9; ++i) G[i] = -G[i];
        double Rt[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rt[3 * i + j] = Xj[3 * j + i];
        m3_mul(Ji, Rt, UL);
        m3_mul(Q2, Rt, LL);
        m3_mul(Ji, G, t1);
        for (int i = 0; i < 9; ++i) LL[i] = LL[i] + t1[i];
        // rows 0..2 of M: [UL, 0]; rows 3..5: [LL, UL]
        auto M = [&](int r, int col) -> double {
            if (r < 3) return col < 3 ? UL[3 * r + col] : 0.0;
            return col < 3 ? LL[3 * (r - 3) + col] : UL[3 * (r - 3) + col - 3];
        };
        double* N = g.N + 36 * (size_t)q;
        double* bv = g.bv + 6 * (size_t)q;
        for (int c1 = 0; c1 < 6; ++c1) {
            double bs = 0.0;
            for (int r = 0; r < 6; ++r) bs = bs + M(r, c1) * (iv[r] * e[r]);
            bv[c1] = w * bs;
            for (int c2 = 0; c2 < 6; ++c2) {
                double ns = 0.0;
                for (int r = 0; r < 6; ++r) ns = ns + M(r, c1) * iv[r] * M(r, c2);
                N[6 * c1 + c2] = w * ns;
            }
        }
        if (KW)
            for (int r = 0; r < 6; ++r) {
                const double sw = sqrt(w * iv[r]);
                for (int c1 = 0; c1 < 6; ++c1) kw[36 * (size_t)q + 6 * r + c1] = sw * M(r, c1);
            }
    }
    for (int q = threadIdx.x; q < g.np; q += kPgoBlock) {
        const double* t = g.X + 12 * (size_t)g.poff[g.n + 1 + q] + 9;
        const double* in = g.pf + 7 * (size_t)q;
        double* work = g.pf + 7 * ((size_t)g.np + q);
        double r[3], iv[3], s2 = 0.0;
        for (int i = 0; i < 3; ++i) {
            r[i] = t[i] - in[i];
            iv[i] = 1.0 / in[3 + i];
            s2 = s2 + r[i] * r[i] * iv[i];
        }
        const double rk = in[6];
        double w = 1.0;
        if (rk > 0.0) {
            const double k2 = rk * rk;
            w = k2 / (k2 + s2);
            cost = cost + 0.5 * k2 * log1p(s2 / k2);
        } else {
            cost = cost + 0.5 * s2;
        }
        for (int i = 0; i < 3; ++i) {
            work[i] = w * iv[i];
            work[3 + i] = w * (iv[i] * r[i]);
        }
        work[6] = w;
    }
    return block_sum(cost, s);
}

}  // namespace ndt
