// ndt_ground.h — filter_node's ground detection (DetectPlane, filter_node.cpp:103-216) on the device: the launch
// constants of ground.hip's kernels, the state of one scan's RANSAC that they hand from launch to launch, and the
// generator table the sampler reads.  Shared by ground.hip (kernels) and host_ground.hip (launches).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "ndt_types.h"

namespace ndt {

constexpr int kGroundBlock = 256;                      // threads per workgroup of every kernel of the unit
constexpr int kGroundTeam = 16;                        // lanes per point of k_ground_normals (knn_walk's team)
constexpr int kGroundTeams = kGroundBlock / kGroundTeam;
constexpr int kGroundNormalMaxBlocks = 8192;           // grid cap of k_ground_normals
constexpr float kGroundCell = 1.0f;                    // cell of the clipped cloud's neighbour index: a 0.5 m-voxel scan has
                                                       // its 10 neighbours within the 3x3x3 cells around a ground point
constexpr int kGroundMaxK = 20;                        // normal_k cap (KnnList<20>)
// Hypotheses per scoring launch.  With a ground share w of the cloud after the normal filter the loop ends after
// k = log(1 - 0.99) / log(1 - w^3) iterations: 7 at w = 0.8, 32 at w = 0.51, so one batch ends almost every scan;
// 32 int counters per lane stay in registers beside the point.
constexpr int kGroundBatch = 32;
constexpr int kGroundChain = 2;                        // (sample, score) pairs per chain of launches, then k_ground_finish
constexpr int kGroundScoreMaxBlocks = 256;             // grid cap of k_ground_score (rows of its partials)
constexpr int kGroundMaxIterations = 4000;             // ransac_max_iterations cap
constexpr int kGroundSampleChecks = 1000;              // SampleConsensusModel::max_sample_checks_
// Words of the generator's stream uploaded per context.  A scan draws 3 words per sample and (max_iterations + 1)
// samples at most, 3003 with the defaults, plus 3 per redraw of a degenerate sample; 4096 leaves 364 redraws, and a
// redraw needs three points whose f32 difference ratios are equal, which measured scans do not contain.  A scan
// that runs past the table is continued from a longer one the host generates (stream_fallbacks counts it).
constexpr int kGroundStreamWords = 4096;

// a sample's status
enum { GROUND_SAMPLE_NONE = -1, GROUND_SAMPLE_DEGENERATE = 0, GROUND_SAMPLE_OK = 1 };

// One scan's RANSAC, device resident.  The host uploads it before the clouds are compacted (n_normal is then written
// by the compaction scan), the sampler and the scoring tails advance it, k_ground_finish closes it.
struct GroundState {
    // ---- set by the host
    int floor_pts, max_it, max_skip, inject;     // gates and caps; inject: the samples are the caller's
    int literal, stream_words, hash_mask, n_input;
    double thr, log_prob, cos_floor;             // distance threshold, log(1 - probability), cos(floor_normal_thresh)
    float ref[4];                                // (T^-1 UnitZ).head3
    // ---- written on the device
    int n_normal;                                // points after the normal filter (compaction scan)
    // sampler: the first three entries of shuffled_indices_, the stream position, samples made, and whether the table ended
    int s[3];
    int stream_pos, made, overrun;
    // the loop
    int best_cnt, best_h, iterations, skipped, seen, done;
    double k;
    // ---- the result record (k_ground_finish)
    int found, reason, n_inliers;
    int winner[3];
    float coeffs[4];
};

// boost::mt19937 (the 32-bit Mersenne twister): the first n outputs for a seed
inline std::vector<uint32_t> mt19937_stream(uint32_t seed, size_t n) {
    uint32_t mt[624];
    mt[0] = seed;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    std::vector<uint32_t> out(n);
    int at = 624;
    for (size_t o = 0; o < n; ++o) {
        if (at == 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            at = 0;
        }
        uint32_t y = mt[at++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        out[o] = y;
    }
    return out;
}

}  // namespace ndt
