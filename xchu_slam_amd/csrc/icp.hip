// icp.hip — point-to-point ICP pass (pcl::IterativeClosestPoint as pgo_node's ICPRefine uses it, pgo_node.cpp:404-483).
//
// One k_icp_pass launch is one ICP iteration:
//   * every workgroup first applies the previous iteration's transform to its points (pcl::transformPointCloud in f32,
//     in place and cumulative, as PCL's loop does) — the apply step fused into the next pass;
//   * CorrespondenceEstimation: the exact nearest target point of each query over ALL target points, by the walk of
//     k_fitness (voxel_build.hip: 16-lane team per query, 3x3x3 cube, 5x5x5 cube, block shells) over the same index,
//     tracking the argmin beside the minimum; equal f32 distances go to the lowest target index in the caller's order
//     (the index build carries that index as a fifth word beside the sorted points);
//   * 17 f64 sums over the kept pairs (n, sum d2, sum p, sum q, sum p q^T), one per lane of the team, reduced per wave,
//     then through LDS, stored as write-through partials; the last workgroup (ticket) sums the partials in index order
//     and runs the rest of the iteration: pair-count test, Umeyama estimate (TransformationEstimationSVD), the final
//     transform, DefaultConvergenceCriteria, the history record.
// A launch that finds the state done returns at once, so fixed-length runs of launches can be one graph.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "ndt_types.h"
#include "ndt_linalg.h"
#include "ndt_icp.h"
#include "ndt_kernels.h"

namespace ndt {

namespace {

constexpr int kIcpU = 8;      // point loads in flight per lane
constexpr int kIcpCells = 2;  // ring-cube cells per lane per step

// running argmin of one lane: squared distance, position in the index, original target index (-2: not loaded yet)
struct Arg {
    float d;
    int pos, orig;
};

// FLANN L2_Simple in f32, as l2_simple of voxel_build.hip
__device__ __forceinline__ float icp_l2(const float4 t, const float q[3]) {
    float d = 0.f, u;
    u = t.x - q[0]; d += u * u;
    u = t.y - q[1]; d += u * u;
    u = t.z - q[2]; d += u * u;
    return d;
}

// candidate j at distance d; a tie goes to the lower original index (loaded only then); a repeated j changes nothing
__device__ __forceinline__ void arg_take(Arg& a, float d, int j, const int* __restrict__ idx) {
    if (d < a.d) {
        a.d = d;
        a.pos = j;
        a.orig = -2;
    } else if (d == a.d && j != a.pos) {
        if (a.orig == -2) a.orig = idx[a.pos];
        const int oj = idx[j];
        if (oj < a.orig) {
            a.pos = j;
            a.orig = oj;
        }
    }
}

// the team's argmin in every lane ((d, orig) is a strict order over distinct points: every lane ends with the same one)
__device__ __forceinline__ void arg_team(Arg& a, const int* __restrict__ idx) {
    if (a.orig == -2) a.orig = idx[a.pos];
    for (int m = kIcpTeam / 2; m > 0; m >>= 1) {
        const float od = __shfl_xor(a.d, m, kIcpTeam);
        const int oo = __shfl_xor(a.orig, m, kIcpTeam);
        const int op = __shfl_xor(a.pos, m, kIcpTeam);
        if (od < a.d || (od == a.d && oo < a.orig)) {
            a.d = od;
            a.orig = oo;
            a.pos = op;
        }
    }
}

// up to kIcpCells cells of a ring cube (cell k0, k0 + kIcpTeam, ...: one lane's share), as cells_min of voxel_build.hip
__device__ __forceinline__ void cells_arg(int k0, int ncell, int side, int ring, const int c[3], const int db[3], const int nbk[3],
                                          const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                          const float4* __restrict__ pts, const int* __restrict__ idx, const float q[3], Arg& a) {
    int occ[kIcpCells], lc[kIcpCells], b[kIcpCells], n[kIcpCells];
#pragma unroll
    for (int i = 0; i < kIcpCells; ++i) {
        const int k = k0 + i * kIcpTeam;
        const int x = c[0] + k % side - ring, y = c[1] + (k / side) % side - ring, z = c[2] + k / (side * side) - ring;
        const bool in = k < ncell && x >= 0 && y >= 0 && z >= 0 && x < db[0] && y < db[1] && z < db[2];
        lc[i] = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
        occ[i] = in ? block_table[((z >> 3) * nbk[1] + (y >> 3)) * nbk[0] + (x >> 3)] : -1;
    }
    int tot = 0;
#pragma unroll
    for (int i = 0; i < kIcpCells; ++i) {
        b[i] = 0;
        n[i] = 0;
        if (occ[i] >= 0) {
            const int* off = cell_off + (size_t)occ[i] * (kFitBlockCells + 1);
            b[i] = off[lc[i]];
            n[i] = off[lc[i] + 1] - b[i];
        }
        tot += n[i];
    }
    for (int j = 0; j < tot; j += kIcpU) {
        float4 p[kIcpU];
        int at[kIcpU];
#pragma unroll
        for (int u = 0; u < kIcpU; ++u) {
            int v = min(j + u, tot - 1);
            int id = 0;
#pragma unroll
            for (int i = 0; i < kIcpCells; ++i) {
                if (v >= 0 && v < n[i]) id = b[i] + v;
                v -= n[i];
            }
            at[u] = id;
            p[u] = pts[id];
        }
#pragma unroll
        for (int u = 0; u < kIcpU; ++u) arg_take(a, icp_l2(p[u], q), at[u], idx);
    }
}

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

// NDT_ICP_WAVES (A/B builds): waves per SIMD the register allocation is held to; unset = the compiler's choice
#ifdef NDT_ICP_WAVES
#define NDT_ICP_OCC __attribute__((amdgpu_waves_per_eu(NDT_ICP_WAVES)))
#else
#define NDT_ICP_OCC
#endif
__global__ __launch_bounds__(kIcpBlock) NDT_ICP_OCC void k_icp_pass(float4* __restrict__ X, int n, IcpState* __restrict__ st,
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
            const float x = T[0] * p.x + T[4] * p.y + T[8] * p.z + T[12];
            const float y = T[1] * p.x + T[5] * p.y + T[9] * p.z + T[13];
            const float z = T[2] * p.x + T[6] * p.y + T[10] * p.z + T[14];
            p = make_float4(x, y, z, p.w);
            if (t == 0) X[i] = p;
        }
        const float q[3] = {p.x, p.y, p.z};
        Arg a = {INFINITY, -1, INT_MAX};
        if (!empty) {
            int c[3];
            for (int k = 0; k < 3; ++k) c[k] = (int)(floorf(q[k] * h->inv_leaf[k]) - (float)h->min_b[k]);
            const float slack = 1e-4f * cell + 4e-7f * (fabsf(q[0]) + fabsf(q[1]) + fabsf(q[2]));
            int r0 = 0, rmax = 0;
            for (int k = 0; k < 3; ++k) {
                const int out = c[k] < 0 ? -c[k] : (c[k] >= db[k] ? c[k] - db[k] + 1 : 0);
                r0 = max(r0, out);
                rmax = max(rmax, max(c[k], db[k] - 1 - c[k]));
            }
            rmax = max(rmax, r0);
            float face = cell;
            for (int k = 0; k < 3; ++k) {
                const float lo = (float)(c[k] + h->min_b[k]) * h->leaf[k];
                face = fminf(face, fminf(fmaxf(q[k] - lo, 0.f), fmaxf(lo + h->leaf[k] - q[k], 0.f)));
            }
            bool done = false;
            // ---- phase 1: the cubes of radius 1 and 2 around the query cell, one cell per lane per step
            if (r0 <= 2) {
                for (int ring = 1; ring <= 2 && !done; ++ring) {
                    const int side = 2 * ring + 1;
                    const int ncell = side * side * side;
                    for (int k0 = t; k0 < ncell; k0 += kIcpCells * kIcpTeam)
                        cells_arg(k0, ncell, side, ring, c, db, nbk, block_table, cell_off, fit_pts, fit_idx, q, a);
                    arg_team(a, fit_idx);
                    // every unvisited point is at least `bound` away; strictly closer than that and no unvisited point can
                    // tie with the match
                    const float bound = fmaxf(0.f, face + (float)ring * cell - slack);
                    done = a.d < bound * bound || ring >= rmax;
                }
            }
            // ---- phase 2: block shells, each candidate block's points split over the team
            if (!done) {
                int cb[3], b0 = 0, bmax = 0;
                for (int k = 0; k < 3; ++k) {
                    cb[k] = c[k] >> 3;  // arithmetic shift: floor for cells left of the grid
                    const int out = cb[k] < 0 ? -cb[k] : (cb[k] >= nbk[k] ? cb[k] - nbk[k] + 1 : 0);
                    b0 = max(b0, out);
                    bmax = max(bmax, max(cb[k], nbk[k] - 1 - cb[k]));
                }
                bmax = max(bmax, b0);
                auto visit_block = [&](int x, int y, int z) {
                    const int occ = block_table[((z * nbk[1] + y) * nbk[0]) + x];
                    if (occ < 0) return;
                    const int bx[3] = {x, y, z};
                    float lb = 0.f;
                    for (int k = 0; k < 3; ++k) {
                        const int lo = bx[k] * 8, hi = lo + 7;
                        const int gap = c[k] < lo ? lo - c[k] - 1 : (c[k] > hi ? c[k] - hi - 1 : 0);
                        const float g = fmaxf(0.f, (float)gap * cell - slack);
                        lb += g * g;
                    }
                    if (lb > a.d) return;  // a is team-uniform here; a block that could only tie is still scanned
                    const int* off = cell_off + (size_t)occ * (kFitBlockCells + 1);
                    const int e = off[kFitBlockCells];
                    for (int j = off[0] + t; j < e; j += kIcpU * kIcpTeam) {
                        float4 pp[kIcpU];
#pragma unroll
                        for (int u = 0; u < kIcpU; ++u) pp[u] = fit_pts[min(j + u * kIcpTeam, e - 1)];
#pragma unroll
                        for (int u = 0; u < kIcpU; ++u) arg_take(a, icp_l2(pp[u], q), min(j + u * kIcpTeam, e - 1), fit_idx);
                    }
                    arg_team(a, fit_idx);
                };
                for (int r = b0; r <= bmax; ++r) {
                    const int lo2 = max(cb[2] - r, 0), hi2 = min(cb[2] + r, nbk[2] - 1);
                    const int lo1 = max(cb[1] - r, 0), hi1 = min(cb[1] + r, nbk[1] - 1);
                    const int lo0 = max(cb[0] - r, 0), hi0 = min(cb[0] + r, nbk[0] - 1);
                    for (int z = lo2; z <= hi2; ++z)
                        for (int y = lo1; y <= hi1; ++y) {
                            if (abs(z - cb[2]) == r || abs(y - cb[1]) == r) {
                                for (int x = lo0; x <= hi0; ++x) visit_block(x, y, z);
                            } else {
                                if (cb[0] - r >= 0) visit_block(cb[0] - r, y, z);
                                if (r > 0 && cb[0] + r <= nbk[0] - 1) visit_block(cb[0] + r, y, z);
                            }
                        }
                    const float bound = fmaxf(0.f, (float)(8 * r) * cell - slack);
                    if (a.d < bound * bound) break;
                }
            }
        }
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
    __shared__ double s_tot[kIcpSums];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    cnt += __shfl_xor(cnt, 16);
    cnt += __shfl_xor(cnt, 32);
    if (lane < kIcpTeam) s_part[wave][lane] = acc;
    if (lane == 0) s_part[wave][16] = (double)cnt;
    __syncthreads();
    const int nb = gridDim.x;
    // partials stored write-through and drained before the ticket, the ticket taker acquires (the hand-off of k_fitness);
    // the storing threads are all lanes of wave 0, whose drain covers them
    if (threadIdx.x < 64) {
        if (threadIdx.x < kIcpSums) {
            double v = s_part[0][threadIdx.x];
            for (int w = 1; w < kWaves; ++w) v += s_part[w][threadIdx.x];
            __hip_atomic_store(partials + (size_t)threadIdx.x * nb + blockIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0)
            s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nb - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- last workgroup: the partials in index order (thread-strided groups of kIcpBlock, then a fixed tree)
    __syncthreads();  // s_part is reused
    for (int k = 0; k < kIcpSums; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += kIcpBlock) v += partials[(size_t)k * nb + b];
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kIcpSums) {
        double v = s_part[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) v += s_part[w][threadIdx.x];
        s_tot[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *ticket = 0u;  // re-armed for the next launch
        double S[kIcpSums];
        for (int k = 0; k < kIcpSums; ++k) S[k] = s_tot[k];
        icp_control(S, st, hist);
    }
}

}  // namespace ndt
