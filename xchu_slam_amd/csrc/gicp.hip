// gicp.hip — Generalized-ICP (pclomp::GeneralizedIterativeClosestPoint, gicp_omp_impl.hpp) on the device.
//
//   k_gicp_cov<C>  computeCovariances (:59-131): one 16-lane team per point over an NNIndex of the point's own cloud.
//                  The walk of k_sor_knn (3x3x3 cube, ring 2, block shells, the same bound); every lane keeps the C
//                  smallest 64-bit keys (d2 bits << 32 | original index) it saw, so the (d2, index) order rule and the
//                  summation order both come out of the merge.  f64 mean and moments in that order, svd_jacobi, rebuild.
//   k_gicp_pairs   one outer iteration's correspondences (:430-463): both transforms, the exact 1-NN walk with the
//                  argmin tracker (ndt_nnwalk.h, as k_icp_pass), the strict threshold, M_i = (R C1 R^T + C2)^-1; its
//                  last workgroup runs gicp_after_pairs.
//   k_gicp_eval    the objective and its gradient (:344-377) at the state's trial transform: 13 f64 sums over the
//                  matched points through a fixed tree, per-workgroup partials, the last workgroup sums them through
//                  a fixed tree too and runs gicp_after_eval (the minimiser step, the next trial transform, the end of a solve).
// A launch whose phase is not the state's current phase returns at its first load.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "ndt_device.h"
#include "ndt_gicp.h"
#include "ndt_nnwalk.h"
#include "ndt_lastwg.h"
#include "ndt_kernels.h"

namespace ndt {

namespace {

static_assert(kGicpTeam == kNnTeam, "k_gicp_pairs' teams are nn_walk's");

constexpr unsigned long long kNoKey = ~0ull;

// The C smallest keys one lane has seen, ascending (registers; branch-free min/max cascade as TopK of front_end.hip)
template <int C>
struct TopKey {
    unsigned long long v[C];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < C; ++j) v[j] = kNoKey;
    }
    __device__ __forceinline__ void insert(unsigned long long d) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const unsigned long long lo = v[j] < d ? v[j] : d;
            d = v[j] < d ? d : v[j];
            v[j] = lo;
        }
    }
    // keys whose distance is strictly below b2
    __device__ __forceinline__ int count_lt(float b2) const {
        int n = 0;
#pragma unroll
        for (int j = 0; j < C; ++j) n += (v[j] != kNoKey && __uint_as_float((unsigned)(v[j] >> 32)) < b2) ? 1 : 0;
        return n;
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int j = 0; j < C - 1; ++j) v[j] = v[j + 1];
        v[C - 1] = kNoKey;
    }
};

__device__ __forceinline__ int gicp_team_sum(int v) {
    for (int m = kGicpTeam / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kGicpTeam);
    return v;
}

// candidate j of the index: its key enters the lane's list when it can be among the C smallest
template <int C>
__device__ __forceinline__ void take(TopKey<C>& top, const float4* __restrict__ ix_pts, const int* __restrict__ ix_idx, int j,
                                     const float q[3]) {
    const float d = nn_l2(ix_pts[j], q);
    const unsigned hi = __float_as_uint(d);
    if (hi > (unsigned)(top.v[C - 1] >> 32)) return;  // d2 >= 0: the bits order as the values
    top.insert(((unsigned long long)hi << 32) | (unsigned)ix_idx[j]);
}

}  // namespace

template <int C>
__global__ __launch_bounds__(kGicpBlock) void k_gicp_cov(const float4* __restrict__ pts, int n, int k, double eps,
                                                         const GridHeader* __restrict__ h, const int* __restrict__ block_table,
                                                         const int* __restrict__ cell_off, const float4* __restrict__ ix_pts,
                                                         const int* __restrict__ ix_idx, double* __restrict__ cov_out,
                                                         double* __restrict__ raw_out) {
    const int db[3] = {h->div_b[0], h->div_b[1], h->div_b[2]};
    const int nbk[3] = {h->nblk[0], h->nblk[1], h->nblk[2]};
    const float cell = h->leaf[0];
    const int t = threadIdx.x % kGicpTeam;
    for (int i = blockIdx.x * kGicpTeams + threadIdx.x / kGicpTeam; i < n; i += gridDim.x * kGicpTeams) {
        const float4 p = pts[i];
        const float q[3] = {p.x, p.y, p.z};
        TopKey<C> top;
        top.init();
        int c[3];
        for (int a = 0; a < 3; ++a) c[a] = (int)(floorf(q[a] * h->inv_leaf[a]) - (float)h->min_b[a]);
        const float slack = 1e-4f * cell + 4e-7f * (fabsf(q[0]) + fabsf(q[1]) + fabsf(q[2]));
        int rmax = 0;
        for (int a = 0; a < 3; ++a) rmax = max(rmax, max(c[a], db[a] - 1 - c[a]));
        bool done = false;
        for (int ring = 1; ring <= 2 && !done; ++ring) {
            const int side = 2 * ring + 1, total = side * side * side;
            for (int kk = t; kk < total; kk += kGicpTeam) {
                const int dx = kk % side - ring, dy = (kk / side) % side - ring, dz = kk / (side * side) - ring;
                if (ring == 2 && abs(dx) < 2 && abs(dy) < 2 && abs(dz) < 2) continue;
                const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                if (x < 0 || y < 0 || z < 0 || x >= db[0] || y >= db[1] || z >= db[2]) continue;
                const int occ = block_table[(((z >> 3) * nbk[1] + (y >> 3)) * nbk[0]) + (x >> 3)];
                if (occ < 0) continue;
                const int l = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
                const int* off = cell_off + (size_t)occ * (kFitBlockCells + 1);
                const int e = off[l + 1];
                for (int j = off[l]; j < e; ++j) take<C>(top, ix_pts, ix_idx, j, q);
            }
            // every unvisited point is at least `bound` away: k visited candidates strictly closer end the search, and
            // no unvisited point can tie with any of them
            const float bound = fmaxf(0.f, (float)ring * cell - slack);
            done = gicp_team_sum(top.count_lt(bound * bound)) >= k || ring >= rmax;
        }
        if (!done) {
            int cb[3], bmax = 0;
            for (int a = 0; a < 3; ++a) {
                cb[a] = c[a] >> 3;
                bmax = max(bmax, max(cb[a], nbk[a] - 1 - cb[a]));
            }
            top.init();  // fresh lists: every point of every visited block exactly once
            for (int r = 0; r <= bmax; ++r) {
                const int lo2 = max(cb[2] - r, 0), hi2 = min(cb[2] + r, nbk[2] - 1);
                const int lo1 = max(cb[1] - r, 0), hi1 = min(cb[1] + r, nbk[1] - 1);
                const int lo0 = max(cb[0] - r, 0), hi0 = min(cb[0] + r, nbk[0] - 1);
                // every block of the cube is tested and the interior skipped: enumerating only the faces (as nn_walk does,
                // three inlined scans) took 130 VGPRs instead of 96 and the target covariances 1.34 ms instead of 1.10
                for (int z = lo2; z <= hi2; ++z)
                    for (int y = lo1; y <= hi1; ++y)
                        for (int x = lo0; x <= hi0; ++x) {
                            if (abs(z - cb[2]) != r && abs(y - cb[1]) != r && abs(x - cb[0]) != r) continue;
                            const int occ = block_table[((z * nbk[1] + y) * nbk[0]) + x];
                            if (occ < 0) continue;
                            const int* off = cell_off + (size_t)occ * (kFitBlockCells + 1);
                            const int e = off[kFitBlockCells];
                            for (int j = off[0] + t; j < e; j += kGicpTeam) take<C>(top, ix_pts, ix_idx, j, q);
                        }
                const float bound = fmaxf(0.f, (float)(8 * r) * cell - slack);
                if (gicp_team_sum(top.count_lt(bound * bound)) >= k) break;
            }
        }
        // merge: k rounds of team argmin over the lane heads (keys are distinct), ascending (d2, index); the sums run in
        // that order, every lane keeping all of them (the neighbour's point is a team-uniform load)
        double mean[3] = {0.0, 0.0, 0.0};
        double c00 = 0.0, c10 = 0.0, c11 = 0.0, c20 = 0.0, c21 = 0.0, c22 = 0.0;
        for (int r = 0; r < k; ++r) {
            unsigned long long m = top.v[0];
            for (int off = kGicpTeam / 2; off > 0; off >>= 1) {
                const unsigned long long om = __shfl_xor(m, off, kGicpTeam);
                m = om < m ? om : m;
            }
            if (m == kNoKey) break;  // fewer than k points in the cloud: the host rejects it before the launch
            if (top.v[0] == m) top.pop();
            const float4 pt = pts[(int)(unsigned)(m & 0xffffffffull)];
            mean[0] += (double)pt.x;
            mean[1] += (double)pt.y;
            mean[2] += (double)pt.z;
            c00 += (double)(pt.x * pt.x);  // f32 products added to f64 sums
            c10 += (double)(pt.y * pt.x);
            c11 += (double)(pt.y * pt.y);
            c20 += (double)(pt.z * pt.x);
            c21 += (double)(pt.z * pt.y);
            c22 += (double)(pt.z * pt.z);
        }
        if (t == 0) {
            const double kd = (double)k;
            for (int a = 0; a < 3; ++a) mean[a] /= kd;
            c00 = c00 / kd - mean[0] * mean[0];
            c10 = c10 / kd - mean[1] * mean[0];
            c11 = c11 / kd - mean[1] * mean[1];
            c20 = c20 / kd - mean[2] * mean[0];
            c21 = c21 / kd - mean[2] * mean[1];
            c22 = c22 / kd - mean[2] * mean[2];
            const double cov[9] = {c00, c10, c20, c10, c11, c21, c20, c21, c22};  // symmetric: either major
            if (raw_out)
                for (int e = 0; e < 9; ++e) raw_out[(size_t)9 * i + e] = cov[e];
            double U[9], V[9], sv[3];
            int nz;
            svd_jacobi<double, 3>(cov, U, V, sv, &nz);
            double out[9];
            for (int e = 0; e < 9; ++e) out[e] = 0.0;
            for (int col = 0; col < 3; ++col) {
                const double v = col == 2 ? eps : 1.0;
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) out[3 * a + b] += (v * U[a + 3 * col]) * U[b + 3 * col];
            }
            for (int e = 0; e < 9; ++e) cov_out[(size_t)9 * i + e] = out[e];  // row-major
        }
    }
}

template __global__ void k_gicp_cov<20>(const float4*, int, int, double, const GridHeader*, const int*, const int*, const float4*,
                                        const int*, double*, double*);
template __global__ void k_gicp_cov<32>(const float4*, int, int, double, const GridHeader*, const int*, const int*, const float4*,
                                        const int*, double*, double*);

__global__ __launch_bounds__(kGicpBlock) void k_gicp_pairs(const float4* __restrict__ src, int n, GicpState* __restrict__ st,
                                                           const GridHeader* __restrict__ h, const int* __restrict__ block_table,
                                                           const int* __restrict__ cell_off, const float4* __restrict__ fit_pts,
                                                           const int* __restrict__ fit_idx, const double* __restrict__ cov_src,
                                                           const double* __restrict__ cov_tgt, int* __restrict__ match,
                                                           float* __restrict__ nn_d2, float4* __restrict__ qt, float4* __restrict__ gp,
                                                           double* __restrict__ Mout, unsigned* __restrict__ ticket,
                                                           GicpRecordDev* __restrict__ hist) {
    // the state is rewritten by this launch's last workgroup only after every workgroup has taken its ticket
    if (st->phase != GICP_PAIRS) return;
    float G[16], T[16];
    for (int k = 0; k < 16; ++k) { G[k] = st->guess[k]; T[k] = st->trans[k]; }
    double R[9];
    for (int k = 0; k < 9; ++k) R[k] = st->Rtg[k];
    const double corr2 = st->corr2;
    const bool empty = h->empty != 0 || h->n_leaves == 0;
    const int db[3] = {h->div_b[0], h->div_b[1], h->div_b[2]};
    const int nbk[3] = {h->nblk[0], h->nblk[1], h->nblk[2]};
    const float cell = h->leaf[0];
    const int t = threadIdx.x % kGicpTeam;
    int cnt = 0;
    for (int i = blockIdx.x * kGicpTeams + threadIdx.x / kGicpTeam; i < n; i += gridDim.x * kGicpTeams) {
        const float4 p = src[i];
        // query = transformation_ * (guess * p), two f32 matrix-vector products
        const float3 g3 = transform_point(G, p.x, p.y, p.z), q3 = transform_point(T, g3.x, g3.y, g3.z);
        const float q[3] = {q3.x, q3.y, q3.z};
        NnArg a = {INFINITY, -1, INT_MAX, fit_idx};
        if (!empty) nn_walk(q, t, h, db, nbk, cell, block_table, cell_off, fit_pts, a);
        const bool keep = a.pos >= 0 && (double)a.d < corr2;  // strict, unlike ICP
        if (t == 0) {
            match[i] = keep ? a.orig : -1;
            nn_d2[i] = a.d;
            gp[i] = make_float4(g3.x, g3.y, g3.z, 1.f);
            if (keep) {
                ++cnt;
                qt[i] = fit_pts[a.pos];
                // M = (R C1 R^T + C2)^-1 in f64, 3-term sums as (a0 b0 + a1 b1) + a2 b2
                const double* C1 = cov_src + (size_t)9 * i;
                const double* C2 = cov_tgt + (size_t)9 * a.orig;
                double RC[9], tmp[9], inv[9];  // RC row-major, tmp / inv column-major
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) RC[3 * r + c] = (R[r] * C1[c] + R[r + 3] * C1[3 + c]) + R[r + 6] * C1[6 + c];
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c)
                        tmp[r + 3 * c] = ((RC[3 * r] * R[c] + RC[3 * r + 1] * R[c + 3]) + RC[3 * r + 2] * R[c + 6]) + C2[3 * r + c];
                inverse3<double>(tmp, inv);
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) Mout[(size_t)9 * i + 3 * r + c] = inv[r + 3 * c];  // row-major
            }
        }
    }
    __shared__ int s_cnt;
    __shared__ int s_last;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt) __hip_atomic_fetch_add(&st->pair_count, s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const int pairs = __hip_atomic_load(&st->pair_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            st->pair_count = 0;
            *ticket = 0u;  // re-armed for the next launch
            gicp_after_pairs(st, hist, pairs);
        }
    }
}

__global__ __launch_bounds__(kGicpBlock) void k_gicp_eval(const float4* __restrict__ src, int n, GicpState* __restrict__ st,
                                                          const int* __restrict__ match, const float4* __restrict__ qt,
                                                          const float4* __restrict__ gp, const double* __restrict__ M,
                                                          double* __restrict__ partials, unsigned* __restrict__ ticket,
                                                          GicpRecordDev* __restrict__ hist) {
    const int phase = st->phase;
    if (phase != GICP_EVAL && phase != GICP_EVAL_ONLY) return;
    float T[16];
    for (int k = 0; k < 16; ++k) T[k] = st->T_trial[k];
    double acc[kGicpSums];
#pragma unroll
    for (int k = 0; k < kGicpSums; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kGicpBlock + threadIdx.x; i < n; i += gridDim.x * kGicpBlock) {
        if (match[i] < 0) continue;
        const float4 p = src[i], q = qt[i], g = gp[i];
        const float3 pt = transform_point(T, p.x, p.y, p.z);
        const double res[3] = {(double)(pt.x - q.x), (double)(pt.y - q.y), (double)(pt.z - q.z)};  // f32 differences widened
        const double* m = M + (size_t)9 * i;
        double tmp[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) tmp[a] = (m[3 * a] * res[0] + m[3 * a + 1] * res[1]) + m[3 * a + 2] * res[2];
        acc[0] += (res[0] * tmp[0] + res[1] * tmp[1]) + res[2] * tmp[2];
        const double gd[3] = {(double)g.x, (double)g.y, (double)g.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[1 + a] += tmp[a];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[4 + 3 * a + b] += gd[a] * tmp[b];
    }
    // ---- a fixed tree: the wave's lanes, the waves in order, then the workgroups' partials (ndt_lastwg.h)
    constexpr int kWaves = kGicpBlock / 64;
    __shared__ double s_part[kWaves][kGicpSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kGicpSums; ++k) {
        double v = acc[k];
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_part[wave][k] = v;
    }
    double S[kGicpSums];
    if (last_workgroup_sums<kGicpSums, kGicpBlock>(s_part, partials, ticket, S)) gicp_after_eval(st, hist, S);
}

}  // namespace ndt
