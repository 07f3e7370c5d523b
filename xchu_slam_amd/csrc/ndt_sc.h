// ndt_sc.h — Scan Context (pgo_node's default loop detector, xchu_mapping/include/scancontext/Scancontext.{h,cpp}) on
// the device: the constants, the database layout and the arithmetic that the kernels of scancontext.hip share.
//
// Semantics are the restatement of DESIGN.md §2 (parity with the reference unpinned: it cannot be compiled here).
// Modelled, not restated: atanf is the f64 arctangent rounded to f32 (the counterpart of sincosf_dr2 in ndt_libm.h);
// every Eigen reduction follows Eigen 3.3's SSE2 order for sizes that are a multiple of four (sc_esum below).
// Non-finite coordinates are outside the contract (filter_node removes them upstream): such points are skipped.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ndt_hip.h"

namespace ndt {

constexpr int kScRings = 20;
constexpr int kScSectors = 60;
constexpr int kScBins = kScRings * kScSectors;  // column-major 20 x 60 as Eigen stores it: bin = sector * 20 + ring
constexpr int kScMaxCand = 16;                  // ndt_sc_result's candidate slots
constexpr int kScBlock = 256;
constexpr int kScMakePerThread = 8;             // points per thread of k_sc_make (2048 per workgroup)
constexpr int kScMakeMaxBlocks = 256;
constexpr double kScMaxRadius = 80.0;
constexpr double kScLidarHeight = 2.0;
constexpr float kScNoPoint = -1000.0f;
constexpr double kScBig = 10000000.0;           // the reference's initial minimum ("something large")

// The database: one slot per keyframe in four arrays (the ring keys on their own: phase 1 of a detection reads only them)
struct ScDb {
    double* desc;      // [cap][1200]
    float* ringkey;    // [cap][20]
    double* sectorkey; // [cap][60]
    double* colnorm;   // [cap][60]
};

struct ScDetectArgs {
    int num_candidates;  // 1..16
    int radius;          // round(0.5 * search_ratio * 60): shifts within it of the sector-key argmin are compared
    double dist_thres;
    int pair_j;          // >= 0: ndt_sc_distance, the one candidate is this slot and phase 1 is skipped
};

// order-preserving uint32 image of an f32 (a < b  <=>  image(a) < image(b), finite values)
__host__ __device__ inline unsigned sc_image(float v) {
    unsigned u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float sc_unimage(unsigned u) {
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}

// max(min(hi, int(ceil(v))), 1); a NaN converts to INT_MIN on x86, which the clamp takes to 1
__host__ __device__ inline int sc_ceil_clamp(double v, int hi) {
    if (!(v == v)) return 1;
    const double c = ceil(v);
    return c < 1.0 ? 1 : (c > (double)hi ? hi : (int)c);
}

// Sum of n (a multiple of four) terms f(0..n-1) in Eigen 3.3's SSE2 linear-vectorised order: four lane sums
// L_k = f(k) + f(k + 4) + ..., then (L0 + L2) + (L1 + L3)
template <typename F> __host__ __device__ inline double sc_esum(int n, F f) {
    double l0 = f(0), l1 = f(1), l2 = f(2), l3 = f(3);
    for (int i = 4; i < n; i += 4) {
        l0 = l0 + f(i);
        l1 = l1 + f(i + 1);
        l2 = l2 + f(i + 2);
        l3 = l3 + f(i + 3);
    }
    return (l0 + l2) + (l1 + l3);
}

}  // namespace ndt
