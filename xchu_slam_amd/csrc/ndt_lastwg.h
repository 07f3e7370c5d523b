// ndt_lastwg.h — the last-workgroup tail of a kernel that ends in K f64 sums over its whole grid (device only): the tail
// of k_icp_pass (icp.hip, K = 17) and of k_gicp_eval (gicp.hip, K = 13).
#pragma once
#include <hip/hip_runtime.h>

namespace ndt {

// Every thread of every workgroup calls it once, with s_part[w][k] = wave w's sum k already written (no barrier yet).
// partials holds K rows of gridDim.x doubles; *ticket is 0 at the launch and is left 0 again.  Returns true in one
// thread only, thread 0 of the last workgroup to arrive, which then holds the grid totals in S and runs the caller's
// control step; false everywhere else (S untouched).  In this form k_icp_pass compiles to the instructions it had with
// the tail written out in the kernel (ten commuted v_mul_f64 operand pairs apart).  Inlined once per kernel: the two
// __shared__ objects below are that kernel's.
// The order of every sum is fixed: the waves of a workgroup in order; over the workgroups thread-strided groups of
// BLOCK in ascending order, then the 64-lane xor tree, then the waves in order.
// Hand-off: the partials are stored write-through (agent-scope relaxed stores) by lanes of wave 0 and drained (vmcnt(0))
// before its lane 0 takes the ticket, so they are in memory before the ticket counts them — an agent-scope release
// fence would write back the whole L2 in each workgroup.  The last workgroup re-reads them with plain loads: its
// agent-scope acquire fence, after the ticket, has invalidated every cached copy a load of this workgroup could hit
// that is not coherent at agent scope (lines of an earlier launch), so the loads behind it see what was drained and
// need no scope of their own (the pass epilogue and k_fitness re-read theirs the same way).
template <int K, int BLOCK>
__device__ __forceinline__ bool last_workgroup_sums(double (*s_part)[K], double* __restrict__ partials, unsigned* __restrict__ ticket,
                                                    double (&S)[K]) {
    static_assert(K <= 64 && BLOCK % 64 == 0, "the K sums of a workgroup are stored by lanes of wave 0");
    constexpr int kWaves = BLOCK / 64;
    __shared__ double s_tot[K];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    const int nb = gridDim.x;
    if (threadIdx.x < 64) {
        if (threadIdx.x < K) {
            double v = s_part[0][threadIdx.x];
            for (int w = 1; w < kWaves; ++w) v += s_part[w][threadIdx.x];
            __hip_atomic_store(partials + (size_t)threadIdx.x * nb + blockIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0)
            s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nb - 1;
    }
    __syncthreads();
    if (!s_last) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // s_part is reused
    for (int k = 0; k < K; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += BLOCK) v += partials[(size_t)k * nb + b];
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double v = s_part[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) v += s_part[w][threadIdx.x];
        s_tot[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    *ticket = 0u;  // re-armed for the next launch
    for (int k = 0; k < K; ++k) S[k] = s_tot[k];
    return true;
}

}  // namespace ndt
