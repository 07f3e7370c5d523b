// fitness.hip — pcl::Registration::getFitnessScore on the device: the exact nearest target point of every transformed
// source point over the target's NNIndex (built by the k_fit_* kernels of voxel_build.hip), the squared distances within
// max_range summed.
#include <hip/hip_runtime.h>
#include "ndt_device.h"
#include "ndt_nnwalk.h"
#include "ndt_kernels.h"

namespace ndt {

// Exact nearest neighbour of each transformed source point (pcl::transformPointCloud in f32) over all target points, one
// 16-lane team per query: nn_walk (ndt_nnwalk.h) with the minimum tracker.
// The per-workgroup (sum, count) partials are summed by the last workgroup to finish (ticket), in a fixed order
// (thread-strided, then a fixed tree), and written straight to the caller's pinned result slots.
// Six waves per SIMD: the search is latency bound (a wave's 4 queries wait on dependent gathers 70 % of the time) and
// 80 VGPRs still need no scratch (C3: 82.8 vs 87.8 us at the default 5 waves; 8 waves spill 76 B/lane, 93 us).
constexpr int kFitWaves = 6;
__global__ __launch_bounds__(kFitBlock) __attribute__((amdgpu_waves_per_eu(kFitWaves))) void k_fitness(const float4* __restrict__ src, int n, Mat4f Tm, const GridHeader* __restrict__ h,
                                                    const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                                    const float4* __restrict__ fit_pts, double max_range, float* __restrict__ nn_d2,
                                                    double* __restrict__ part_sum, int* __restrict__ part_cnt,
                                                    unsigned* __restrict__ ticket, double* __restrict__ out_sum,
                                                    long long* __restrict__ out_cnt) {
    const float* T = Tm.m;
    double sum = 0.0;
    int cnt = 0;
    const bool empty = h->empty != 0 || h->n_leaves == 0;
    const int db[3] = {h->div_b[0], h->div_b[1], h->div_b[2]};
    const int nbk[3] = {h->nblk[0], h->nblk[1], h->nblk[2]};
    const float cell = h->leaf[0];
    const int t = threadIdx.x % kNnTeam;
    const int teams = kFitBlock / kNnTeam;
    for (int i = blockIdx.x * teams + threadIdx.x / kNnTeam; i < n; i += gridDim.x * teams) {
        const float4 p = src[i];
        const float3 x3 = transform_point(T, p.x, p.y, p.z);
        const float q[3] = {x3.x, x3.y, x3.z};
        NnMin best = {INFINITY};
        if (!empty) nn_walk(q, t, h, db, nbk, cell, block_table, cell_off, fit_pts, best);
        if (t == 0) {
            nn_d2[i] = best.d;
            if (best.d != INFINITY && (double)best.d <= max_range) { sum += (double)best.d; ++cnt; }
        }
    }
    // (sum, count): workgroup tree -> per-workgroup partial; the last workgroup of each group of kFitGroup sums its
    // group's partials (one load per thread, fixed tree) into a group partial; the last group's reducer sums the
    // group partials (fixed tree) into the caller's pinned result slots.  Hand-offs as in the pass epilogue (recipe
    // R1): partials stored write-through (sc1) and drained before the ticket, the ticket taker acquires — an
    // agent-scope release fence would write back the L2 in each of thousands of workgroups.  One counter per group
    // (own cache line): thousands of increments of one word serialise at its L2 channel.
    __shared__ double s_sum[kFitBlock];
    __shared__ long long s_cnt[kFitBlock];
    __shared__ int s_role;
    auto tree = [&](double v, long long k) {
        s_sum[threadIdx.x] = v;
        s_cnt[threadIdx.x] = k;
        __syncthreads();
        for (int off = kFitBlock / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) { s_sum[threadIdx.x] += s_sum[threadIdx.x + off]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + off]; }
            __syncthreads();
        }
    };
    tree(sum, cnt);
    const int nb = gridDim.x;
    const int g = blockIdx.x / kFitGroup, ng = (nb + kFitGroup - 1) / kFitGroup;
    const int g0 = g * kFitGroup, gsize = min(kFitGroup, nb - g0);
    if (threadIdx.x == 0) {
        __hip_atomic_store(part_sum + blockIdx.x, s_sum[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part_cnt + blockIdx.x, (int)s_cnt[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_role = __hip_atomic_fetch_add(&ticket[kFitTicketStride * (1 + g)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                 (unsigned)gsize - 1;
    }
    __syncthreads();
    if (!s_role) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    {
        const int t = threadIdx.x;
        tree(t < gsize ? part_sum[g0 + t] : 0.0, t < gsize ? (long long)part_cnt[g0 + t] : 0ll);
    }
    if (threadIdx.x == 0) {
        ticket[kFitTicketStride * (1 + g)] = 0u;
        __hip_atomic_store(part_sum + nb + g, s_sum[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part_cnt + nb + g, (int)s_cnt[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_role = __hip_atomic_fetch_add(&ticket[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)ng - 1 ? 2 : 0;
    }
    __syncthreads();
    if (s_role != 2) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    {
        // more groups than threads: each thread first sums its strided share in ascending order (fixed order)
        double v = 0.0;
        long long k = 0;
        for (int t = threadIdx.x; t < ng; t += kFitBlock) { v += part_sum[nb + t]; k += part_cnt[nb + t]; }
        tree(v, k);
    }
    if (threadIdx.x == 0) {
        // pinned host slots: system-scope stores; a count of -1 reports an index whose sort hit the look-back time limit
        // (the header's error flag: the decoupled look-backs rely on each XCD dispatching its workgroups in order)
        __hip_atomic_store(out_sum, s_sum[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(out_cnt, h->pad[0] ? -1ll : (long long)s_cnt[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        ticket[0] = 0u;
    }
}

}  // namespace ndt
