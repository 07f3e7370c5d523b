// ndt_map.h — the global map (pgo_node's SaveMap, PublishPoseAndFrame and LoopFindNearKeyframesCloud: keyframes moved by
// their poses, stacked, pcl::VoxelGrid) on the device: the launch constants of k_map_stack (keyframe_map.hip), the
// per-point arithmetic it shares with k_transform_mat (solver.hip), and the host arithmetic of a selection's table.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "ndt_types.h"

namespace ndt {

constexpr int kMapPointsPerWg = 4 * kBlock;  // output points a k_map_stack workgroup takes at a time (16 KiB in, 16 KiB out)
constexpr int kMapMaxBlocks = 2048;          // grid cap (8 workgroups on each of 256 CUs); the rest is strided

// pcl::transformPointCloud for one PointXYZI: ((T0 x + T4 y) + T8 z) + T12 per row of the column-major T, the 4th lane
// (intensity) carried through.  The one expression k_transform_mat and k_map_stack evaluate (-ffp-contract=off: no
// fused multiply-add), so a stacked map equals per-keyframe ndt_transform_device bit for bit.
__device__ __forceinline__ float4 transform_point_mat(const Mat4f& T, float4 p) {
    float4 o;
    o.x = T.m[0] * p.x + T.m[4] * p.y + T.m[8] * p.z + T.m[12];
    o.y = T.m[1] * p.x + T.m[5] * p.y + T.m[9] * p.z + T.m[13];
    o.z = T.m[2] * p.x + T.m[6] * p.y + T.m[10] * p.z + T.m[14];
    o.w = p.w;
    return o;
}

// Launch geometry of k_map_stack for `total` output points: workgroups (each strides over tiles of kMapPointsPerWg)
inline int map_stack_blocks(long long total) {
    const long long tiles = (total + kMapPointsPerWg - 1) / kMapPointsPerWg;
    return (int)(tiles < 1 ? 1 : tiles > kMapMaxBlocks ? kMapMaxBlocks : tiles);
}

// The exclusive prefix of a selection's keyframe counts (n_sel + 1 entries, prefix[n_sel] = the stacked size) as a
// 64-bit sum; index NULL selects 0..n_sel-1.  Returns false at the first index outside [0, size).
inline bool map_selection_prefix(const std::vector<long long>& count, const int* index, int n_sel, std::vector<long long>& prefix) {
    prefix.assign((size_t)n_sel + 1, 0);
    for (int k = 0; k < n_sel; ++k) {
        const int i = index ? index[k] : k;
        if (i < 0 || (size_t)i >= count.size()) return false;
        prefix[(size_t)k + 1] = prefix[(size_t)k] + count[(size_t)i];
    }
    return true;
}

}  // namespace ndt
