// ndt_isc.h — Intensity Scan Context (pgo_node's loop_method 2, xchu_mapping/include/isc/ISCGeneration.{h,cpp}) on the
// device: the constants, the database layout and the arithmetic that the kernels of isc.hip share.
//
// Semantics are the restatement of DESIGN.md §2 "ISC" (parity with the reference unpinned: it cannot be compiled here).
// Modelled, not restated: atan2f is the f64 arctangent rounded to f32 (as Scan Context's atanf, ndt_sc.h); Eigen's
// three-term sums follow Eigen 3.3's SSE2 order, (x + y) + z.  Deviations, each where the reference leaves its row or is
// order-dependent: a negative sector index is skipped, an intensity outside 0..1 clamps to 0..255 (NaN: 0), and the
// intensity window wraps its column with a true modulo.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ndt_hip.h"

namespace ndt {

constexpr int kIscMaxRings = 64;      // a column's rings fit one 64-bit mask
constexpr int kIscMaxSectors = 128;   // the +-10-column intensity window never wraps twice (sectors >= 20)
constexpr int kIscMinSectors = 20;
constexpr int kIscColBytes = 64;      // a stored column: `rings` bytes, zero-padded to 64
constexpr int kIscColWords = kIscColBytes / 4;
constexpr int kIscBlock = 256;
constexpr int kIscMakePerThread = 8;  // points per thread of k_isc_make (2048 per workgroup)
constexpr int kIscMakeMaxBlocks = 256;
constexpr int kIscChunk = 64;         // candidates per workgroup of k_isc_detect (one gate per thread of wave 0)
constexpr int kIscWindow = 10;        // calculate_intensity_dis: the shifts angle - 10 .. angle + 9

// The database, sector-major: slot k holds `sectors` columns of 64 bytes (a column shift is an aligned whole-column move)
// and per column the ring masks "cell == 0" and "cell == 1" (bits 0 .. rings-1), which is all calculate_geometry_dis
// compares; then the keyframe position (narrowed through f32, as pcl::PointXYZI holds it) and the travel distance.
struct IscDb {
    unsigned char* cols;         // [cap][sectors][64]
    unsigned long long* zero;    // [cap][sectors]
    unsigned long long* one;     // [cap][sectors]
    double* pos;                 // [cap][3]
    double* travel;              // [cap]
};

struct IscGeom {
    int rings, sectors;
    double max_dis, ring_step, sector_step;
    float z_min, z_max;
};

struct IscDetectArgs {
    int rings, sectors;
    double skip_distance, inflation, geo_thres, inten_thres;
    int n_chunks;      // workgroups per query
    int pair_j;        // >= 0: ndt_isc_pair, the one candidate is this slot, ungated, and the intensity is always computed
    int pair_angle;    // pair mode: >= 0 evaluates the intensity window around this shift instead of the geometry's
};

// One workgroup's share of a query: its best passing pair under "greater sum, or equal sum and lower index", and its counts
struct IscPartial {
    double sum, geo, inten;      // sum == 0: no passing pair
    int idx, angle;
    int n_gated, n_geo, n_loop;
    int pad;
};

// (int)(255.f * intensity) stored in a byte: clamped to 0..255, NaN as 0 (within the contract 0 <= intensity <= 1 the
// reference's value)
__host__ __device__ inline int isc_intensity(float w) {
    const float v = 255.f * w;
    if (!(v == v) || v <= 0.f) return 0;
    return v >= 255.f ? 255 : (int)v;
}

// a replaces b as the best pair: the reference's ascending scan with a strict >
__host__ __device__ inline bool isc_better(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && sa > 0.0 && ia < ib); }

}  // namespace ndt
