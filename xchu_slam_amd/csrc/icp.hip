// icp.hip — point-to-point ICP pass (pcl::IterativeClosestPoint as pgo_node's ICPRefine uses it, pgo_node.cpp:404-483).
//
// One k_icp_pass launch is one ICP iteration:
//   * every workgroup first applies the previous iteration's transform to its points (pcl::transformPointCloud in f32,
//     in place and cumulative, as PCL's loop does) — the apply step fused into the next pass;
//   * CorrespondenceEstimation: the exact nearest target point of each query over ALL target points, by the walk
//     k_fitness uses (ndt_nnwalk.h: 16-lane team per query, 3x3x3 cube, 5x5x5 cube, block shells) over the same index,
//     with the argmin tracker; equal f32 distances go to the lowest target index in the caller's order (the index
//     build carries that index as a fifth word beside the sorted points);
//   * 17 f64 sums over the kept pairs (n, sum d2, sum p, sum q, sum p q^T), one per lane of the team, reduced per wave,
//     then through LDS, stored as write-through partials; the last workgroup (ticket, ndt_lastwg.h) sums the partials in
//     index order and runs the rest of the iteration: pair-count test, Umeyama estimate (TransformationEstimationSVD),
//     the final transform, DefaultConvergenceCriteria, the history record.
// A launch that finds the state done returns at once, so fixed-length runs of launches can be one graph.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "ndt_device.h"
#include "ndt_icp.h"
#include "ndt_nnwalk.h"
#include "ndt_lastwg.h"
#include "ndt_kernels.h"

namespace ndt {

namespace {

static_assert(kIcpTeam == kNnTeam, "k_icp_pass's teams are nn_walk's");

__device__ __forceinline__ double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2]) + m[6] * (m[1] * m[5] - m[4] * m[2]);
}

// Steps 2-5 of one iteration from the 17 sums S (one thread of the last workgroup).
__device__ void icp_control(const double* S, IcpState* st, IcpRecordDev* hist) {
    const int n = (int)S[16];
    const double mse = n > 0 ? S[0] / (double)n : 0.0;
    float Tn[16];
    for (int k = 0; k < 16; ++k) Tn[k] = (k % 5 == 0) ? 1.f : 0.f;
    st->pairs = n;
    st->mse = mse;
    int conv = ICP_NOT_CONVERGED;
    if (n < st->min_pairs) {
        // too few correspondences: the final transform stays as it was
        conv = ICP_NO_CORRESPONDENCES;
        st->converged = 0;
        st->done = 1;
    } else {
        // TransformationEstimationSVD (Umeyama without scale), f64: sigma = 1/n sum (q - qm)(p - pm)^T = U S V^T
        const double inv = 1.0 / (double)n;
        double pm[3], qm[3], sigma[9], U[9], V[9], sv[3], R[9];
        for (int a = 0; a < 3; ++a) { pm[a] = S[1 + a] * inv; qm[a] = S[4 + a] * inv; }
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 3; ++i) sigma[i + 3 * j] = (S[7 + 3 * j + i] - (double)n * qm[i] * pm[j]) * inv;
        int nz;
        svd_jacobi<double, 3>(sigma, U, V, sv, &nz);
        const double sgn = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 3; ++i)
                R[i + 3 * j] = (U[i] * V[j] + U[i + 3] * V[j + 3]) + sgn * (U[i + 6] * V[j + 6]);
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 3; ++i) Tn[i + 4 * j] = (float)R[i + 3 * j];
        for (int i = 0; i < 3; ++i) Tn[12 + i] = (float)(qm[i] - ((R[i] * pm[0] + R[i + 3] * pm[1]) + R[i + 6] * pm[2]));
        // final_transformation_ = T * final_transformation_ (Matrix4f product)
        float F[16];
        for (int k = 0; k < 16; ++k) F[k] = st->final_tf[k];
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 4; ++i)
                st->final_tf[i + 4 * j] = ((Tn[i] * F[4 * j] + Tn[i + 4] * F[4 * j + 1]) + Tn[i + 8] * F[4 * j + 2]) + Tn[i + 12] * F[4 * j + 3];
        for (int k = 0; k < 16; ++k) st->T[k] = Tn[k];
        st->apply = 1;
        const int it = ++st->iterations;
        // DefaultConvergenceCriteria, first match wins
        const double cos_angle = 0.5 * (((double)Tn[0] + (double)Tn[5] + (double)Tn[10]) - 1.0);
        const double tsq = ((double)Tn[12] * (double)Tn[12] + (double)Tn[13] * (double)Tn[13]) + (double)Tn[14] * (double)Tn[14];
        const double prev = st->prev_mse;
        if (it >= st->max_iter) conv = ICP_ITERATIONS;
        else if (st->trans_eps > 0.0 && cos_angle >= 1.0 - st->trans_eps && tsq <= st->trans_eps) conv = ICP_TRANSFORM;
        else if (fabs(mse - prev) < 1e-12) conv = ICP_ABS_MSE;
        else if (st->fit_eps > 0.0 && fabs(mse - prev) / prev < st->fit_eps) conv = ICP_REL_MSE;
        else st->prev_mse = mse;
        if (conv != ICP_NOT_CONVERGED) {
            st->converged = 1;
            st->done = 1;
        }
    }
    st->conv_state = conv;
    const int hc = st->hist_count;
    if (hc < kIcpMaxHistory) {
        IcpRecordDev* r = hist + hc;
        for (int k = 0; k < 16; ++k) r->T[k] = Tn[k];
        r->mse = mse;
        r->pairs = n;
        r->conv_state = conv;
    }
    st->hist_count = hc + 1;
}

}  // namespace

__global__ __launch_bounds__(kIcpBlock) void k_icp_pass(float4* __restrict__ X, int n, IcpState* __restrict__ st,
                                                        const GridHeader* __restrict__ h, const int* __restrict__ block_table,
                                                        const int* __restrict__ cell_off, const float4* __restrict__ fit_pts,
                                                        const int* __restrict__ fit_idx, int* __restrict__ match,
                                                        float* __restrict__ nn_d2, double* __restrict__ partials,
                                                        unsigned* __restrict__ ticket, IcpRecordDev* __restrict__ hist) {
    // the state is rewritten by this launch's last workgroup only after every workgroup has taken its ticket
    if (st->done) return;
    const bool apply = st->apply != 0;
    float T[16];
    for (int k = 0; k < 16; ++k) T[k] = st->T[k];
    const double max_corr2 = st->max_corr2;
    const bool empty = h->empty != 0 || h->n_leaves == 0;
    const int db[3] = {h->div_b[0], h->div_b[1], h->div_b[2]};
    const int nbk[3] = {h->nblk[0], h->nblk[1], h->nblk[2]};
    const float cell = h->leaf[0];
    const int t = threadIdx.x % kIcpTeam;
    // lane t of a team keeps sum t: 0 d2, 1-3 p, 4-6 q, 7-15 p[a] q[b] (a = (t - 7) / 3, b = (t - 7) % 3), each term A * B
    // with A in {d2, p, 1} and B in {q, 1} (f64 products of f32 values: exact); the pair count is kept by every lane
    const int ia = t == 0 ? 3 : (t < 4 ? t - 1 : (t < 7 ? -1 : (t - 7) / 3));
    const int ib = t < 4 ? -1 : (t < 7 ? t - 4 : (t - 7) % 3);
    double acc = 0.0;
    int cnt = 0;
    for (int i = blockIdx.x * kIcpTeams + threadIdx.x / kIcpTeam; i < n; i += gridDim.x * kIcpTeams) {
        float4 p = X[i];
        if (apply) {
            const float3 x3 = transform_point(T, p.x, p.y, p.z);
            p = make_float4(x3.x, x3.y, x3.z, p.w);
            if (t == 0) X[i] = p;
        }
        const float q[3] = {p.x, p.y, p.z};
        NnArg a = {INFINITY, -1, INT_MAX, fit_idx};
        if (!empty) nn_walk(q, t, h, db, nbk, cell, block_table, cell_off, fit_pts, a);
        const bool keep = a.pos >= 0 && (double)a.d <= max_corr2;
        if (t == 0) {
            match[i] = keep ? a.orig : -1;
            nn_d2[i] = a.d;
        }
        if (keep) {
            const float4 m = fit_pts[a.pos];
            const double A = ia == 3 ? (double)a.d : (ia == 0 ? (double)p.x : (ia == 1 ? (double)p.y : (ia == 2 ? (double)p.z : 1.0)));
            const double B = ib == 0 ? (double)m.x : (ib == 1 ? (double)m.y : (ib == 2 ? (double)m.z : 1.0));
            acc += A * B;
            ++cnt;
        }
    }
    // ---- per wave: the four teams' sums (lanes t, t + 16, t + 32, t + 48), then the waves through LDS in wave order
    constexpr int kWaves = kIcpBlock / 64;
    __shared__ double s_part[kWaves][kIcpSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    cnt += __shfl_xor(cnt, 16);
    cnt += __shfl_xor(cnt, 32);
    if (lane < kIcpTeam) s_part[wave][lane] = acc;
    if (lane == 0) s_part[wave][16] = (double)cnt;
    // ---- the workgroups' partials, summed in index order by the last workgroup, whose thread 0 runs the rest
    double S[kIcpSums];
    if (last_workgroup_sums<kIcpSums, kIcpBlock>(s_part, partials, ticket, S)) icp_control(S, st, hist);
}

}  // namespace ndt
