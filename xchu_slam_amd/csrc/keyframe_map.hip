// keyframe_map.hip — k_map_stack: any selection of the keyframe store's clouds, each moved by its own pose, stacked in
// selection order in one launch (the cloud pgo_node's SaveMap :620-653, PublishPoseAndFrame :744-812 and
// LoopFindNearKeyframesCloud :530-554 hand to pcl::VoxelGrid).
#include "ndt_kernels.h"

namespace ndt {

// A workgroup owns the output points [tile * per_wg, (tile + 1) * per_wg) of every tile it strides to.  prefix is the
// exclusive prefix of the selected keyframes' counts (n_seg + 1 entries, prefix[n_seg] = total), seg_off a segment's
// first point in the arena, seg_T its pose.  The workgroup finds the segment of its first point by a binary search
// over prefix (uniform across the workgroup: scalar loads, no LDS; a later tile searches from the segment the previous
// one ended in), then walks across segment boundaries; empty segments own no output point and are stepped over.  Per
// point one 16-byte load and one 16-byte store.
__global__ __launch_bounds__(kBlock) void k_map_stack(const float4* __restrict__ arena, const int* __restrict__ prefix,
                                                      const long long* __restrict__ seg_off, const Mat4f* __restrict__ seg_T, int n_seg,
                                                      int total, int per_wg, float4* __restrict__ out) {
    int s_from = 0;
    for (long long base = (long long)blockIdx.x * per_wg; base < total; base += (long long)gridDim.x * per_wg) {
        int lo = (int)base;
        const int hi = (int)(base + per_wg < total ? base + per_wg : total);
        // the segment s with prefix[s] <= lo < prefix[s + 1]: the last entry of prefix[s_from .. n_seg) that is <= lo
        // (prefix[s_from] <= lo holds: 0 at first, later the segment an earlier tile of this workgroup reached)
        int a = s_from, b = n_seg;
        while (b - a > 1) {
            const int mid = a + (b - a) / 2;
            if (prefix[mid] <= lo) a = mid; else b = mid;
        }
        int s = a;
        while (lo < hi && s < n_seg) {
            const int seg_begin = prefix[s], seg_end = prefix[s + 1];
            const int end = seg_end < hi ? seg_end : hi;
            if (lo < end) {
                const Mat4f T = seg_T[s];
                const float4* __restrict__ src = arena + seg_off[s];
                // 64-bit: lo + threadIdx.x + kBlock may pass 2^31 - 1 in the last tile of the largest legal selection
                for (long long i = (long long)lo + threadIdx.x; i < end; i += kBlock) out[i] = transform_point_mat(T, src[i - seg_begin]);
                lo = end;
            }
            if (lo < hi) ++s;
        }
        s_from = s < n_seg ? s : n_seg - 1;
    }
}

}  // namespace ndt
