// ndt_geom.h — launch geometry of the derivative passes as pure host functions of a small POD (PassShape): which
// k_pass_direct / k_pass_lead instantiation a context launches, over how many workgroups, with how many points per
// workgroup and tile, and how a grid's partials are summed (one level, or the two-level hand-off of pass_handoff).
// Beside it the two host steps every unit shares: the grid size of a capped launch (grid_for) and the packing of a
// caller's strided cloud into 4-float points (pack_cloud4, xyzi_layout_ok).
// No HIP dependency: host_align.hip launches through it, ndt_pass_geometry reports from it, and
// tests/native/pass_geom_check.cpp and cloud_pack_check.cpp run it with a host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>
#ifndef __host__  // a host compiler: ndt_types.h marks its constexpr helpers for both sides
#define __host__
#define __device__
#endif
#include "ndt_types.h"

namespace ndt::host {

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// What the pass geometry of a context depends on: its share of compute units, the source and target sizes, the
// neighbourhood search (SearchMode), VGC's minimum points per voxel and ndt_set_pass_options' points_per_thread
struct PassShape {
    int n_cu, N, M, search, min_points_per_voxel, ppt;
};

// Workgroups of a grid-stride launch over n items, `per` items per workgroup and round: at least one, at most cap
inline int grid_for(long long n, long long per, int cap) { return (int)std::max(1LL, std::min((n + per - 1) / per, (long long)cap)); }

// k_pass_radius: one point per thread, grid-stride, at most 2048 workgroups
inline int pass_blocks(int n) { return grid_for(n, kBlock, 2048); }

// The layout rule of the C-ABI's xyzi clouds: records of at least four floats, the intensity behind xyz and inside the record
inline bool xyzi_layout_ok(size_t stride_bytes, int intensity_offset) {
    return stride_bytes >= 16 && intensity_offset >= 3 && (size_t)intensity_offset * 4 + 4 <= stride_bytes;
}

// n records of stride_bytes, each starting with x, y, z, packed into 4-float points (x, y, z, w): w the record's float
// at intensity_offset, or 1.0f when intensity_offset < 0 (an xyz cloud).  Only packs: the upload and its synchronise
// stay with the caller, which keeps the vector until then.
inline std::vector<float> pack_cloud4(const void* records, size_t n, size_t stride_bytes, int intensity_offset) {
    std::vector<float> out(4 * n);
    const char* base = static_cast<const char*>(records);
    for (size_t i = 0; i < n; ++i) {
        const char* rec = base + i * stride_bytes;
        std::memcpy(&out[4 * i], rec, 3 * sizeof(float));
        if (intensity_offset < 0) out[4 * i + 3] = 1.0f;
        else std::memcpy(&out[4 * i + 3], rec + (size_t)intensity_offset * sizeof(float), sizeof(float));
    }
    return out;
}

// The point count a pass chain's launch geometry is built for: the scan's size rounded up to 1/64 of its power of two
// (<= ~1.6 % more points per workgroup), at least a multiple of 256.  The pass kernels take the real count from the align state, so one
// captured chain serves every scan of the bucket: odom_node's filtered scans change size every frame, and a chain
// re-captured per align cost ~50 us (4 k points, 11 passes: 0.226 vs 0.178 ms per align).  Source buffers hold at least
// this many points (the kernels prefetch up to it).
inline int geom_points(int n) {
    if (n <= 4096) return std::max(256, ceil_div(n, 256) * 256);
    int p = 1;
    while (p * 2 <= n) p *= 2;
    const int step = p / 64;
    return ceil_div(n, step) * step;
}

// Direct-pass geometry: one workgroup per CU (fewer for small clouds), each taking `rounds` tiles of ppb points
// (ppb <= the workgroup size) so every CU carries the same share of the scan.
struct PassGeom {
    int nb, ppb, block;
};

// Workgroups of at most one per CU (of this ctx's share) x the pass's workgroups per CU, and at least ~64 points each
inline int direct_blocks(const PassShape& s, bool lead, int n, int ppt) {
    return std::max(1, std::min(s.n_cu * pass_wgs_per_cu(s.search, lead, ppt), ceil_div(n, 64)));
}

// Last-workgroup-tail passes of large clouds as a grid of one-tile workgroups (k_pass_direct<S, 1, true>: no tile loop,
// three waves per SIMD, as many 256-point workgroups as the scan needs — C5's 1 M points: 3 907) whose partials are
// summed by the two-level hand-off (pass_handoff); the alternative to the two-points-per-thread tile loop (pass_ppt2).
// ndt_set_pass_options(points_per_thread = 3) selects it (A/B; off by default).
inline bool grid_one_tile(const PassShape& s) {
    if (s.ppt != 3 || s.search == S_DIRECT26) return false;
    return geom_points(std::max(1, s.N)) > s.n_cu * kLeadBlock1;
}

// Last-workgroup-tail passes (k_pass_direct) of DIRECT7 / DIRECT1 hold two points per thread in a tile (half the
// tiles, the pair list packed into one word) once a workgroup walks >= 4 tiles of one point per thread (C5's 1 M-point
// scans: pass 87 -> 81 us; at C4's 3 tiles the halved tile count loses, 27.4 -> 28.8 us).  Every cloud index must then
// fit 22 bits.  ndt_set_pass_options(points_per_thread = 1) keeps one point per thread.
inline bool pass_ppt2(const PassShape& s) {
    if (s.ppt != 2 || s.search == S_DIRECT26 || grid_one_tile(s)) return false;
    const long long max_cloud = (long long)s.M / std::max(1, s.min_points_per_voxel) + 1;
    const int n = geom_points(std::max(1, s.N));
    const int rounds1 = ceil_div(n, direct_blocks(s, false, n, 1) * pass_block(s.search, false));
    return max_cloud < (1ll << 22) && rounds1 >= 4;
}

// leading-tail passes in one tile per workgroup (k_pass_lead<S, true>): DIRECT7 / DIRECT1 whose point bucket fits one
// 768-point tile per CU
inline bool lead_one_tile(const PassShape& s) {
    return s.search != S_DIRECT26 && (long long)geom_points(std::max(1, s.N)) <= (long long)s.n_cu * kLeadBlock1;
}

inline PassGeom direct_geom(const PassShape& s, bool lead) {
    PassGeom g;
    g.block = pass_block(s.search, lead, lead && lead_one_tile(s));
    const int n = geom_points(std::max(1, s.N));
    if (!lead && grid_one_tile(s)) {
        g.nb = ceil_div(n, g.block);
        g.ppb = g.block;
        return g;
    }
    const int ppt = (!lead && pass_ppt2(s)) ? 2 : 1;
    g.nb = direct_blocks(s, lead, n, ppt);
    const int per_tile = g.block * ppt;
    const int rounds = ceil_div(n, g.nb * per_tile);
    g.ppb = ceil_div(n, g.nb * rounds);
    return g;
}

// The launch a context makes, for ndt_pass_geometry: which = 0 k_pass_direct, 1 k_pass_lead, 2 k_pass_radius.
// out: [0] workgroups, [1] block size, [2] points per workgroup and tile (ppb), [3] points per thread, [4] one-tile
// kernel, [5] tiles per workgroup, [6] groups of the two-level hand-off (0: one level), [7] workgroups per group.
// A leading-tail kernel has no hand-off (every workgroup sums the previous pass's partials itself).
inline bool describe_pass(const PassShape& s, int which, int out[8]) {
    if (which < 0 || which > 2) return false;
    const int n = geom_points(std::max(1, s.N));
    if (which == 2) {
        out[0] = pass_blocks(n);
        out[1] = out[2] = kBlock;
        out[3] = 1;
        out[4] = 0;
    } else {
        const bool lead = which == 1;
        const PassGeom g = direct_geom(s, lead);
        out[0] = g.nb;
        out[1] = g.block;
        out[2] = g.ppb;
        out[3] = (!lead && pass_ppt2(s)) ? 2 : 1;
        out[4] = (lead ? lead_one_tile(s) : grid_one_tile(s)) ? 1 : 0;
    }
    out[5] = ceil_div(n, (long long)out[0] * out[2]);
    const bool two = which != 1 && out[0] > kTwoLevelMinBlocks;
    out[7] = two ? group_size(out[0]) : 0;
    out[6] = two ? ceil_div(out[0], out[7]) : 0;
    return true;
}

}  // namespace ndt::host
