// ndt_icp.h — device-resident state of the point-to-point ICP operator (icp.hip, host_icp.hip).
//
// pcl::IterativeClosestPoint as pgo_node's PGO::ICPRefine drives it (pgo_node.cpp:404-483): one k_icp_pass launch per
// iteration, the whole control flow (pair count test, Umeyama estimate, final transform, convergence criteria) in the
// last workgroup of the pass, so a run of passes is one graph launch and the host reads IcpState once per run.
#pragma once
#include "ndt_types.h"

namespace ndt {

constexpr int kIcpBlock = 256;                     // threads per k_icp_pass workgroup
constexpr int kIcpTeam = kFitTeam;             // lanes per query (the k_fitness team)
constexpr int kIcpTeams = kIcpBlock / kIcpTeam;    // queries per workgroup step
constexpr int kIcpMaxBlocks = 1024;                // grid cap: the tail reads 17 partials per workgroup
constexpr int kIcpSums = 17;                       // sum d2, sum p[3], sum q[3], sum p q^T [9], n
constexpr int kIcpMaxHistory = 4096;               // per-iteration records kept (later iterations run unrecorded)

// ndt_icp_state of include/ndt_hip.h
enum IcpConv { ICP_NOT_CONVERGED = 0, ICP_ITERATIONS = 1, ICP_TRANSFORM = 2, ICP_ABS_MSE = 3, ICP_REL_MSE = 4,
               ICP_NO_CORRESPONDENCES = 5 };

struct IcpState {
    // ---- constants of this align ----
    double max_corr2;       // max_corr_dist^2 (a pair is kept when (double)d2 <= max_corr2)
    double trans_eps;       // transformation_epsilon (0: test off)
    double fit_eps;         // euclidean_fitness_epsilon (0: test off)
    int max_iter, min_pairs;
    // ---- state ----
    int done, converged, conv_state, iterations;
    int apply;              // the next pass applies T to its points first (the previous estimate, or a non-identity guess)
    int pairs;              // pairs of the last pass
    int hist_count;
    int pad;
    double mse, prev_mse;
    float T[16];            // the transform the next pass applies (column-major)
    float final_tf[16];     // final_transformation_
};

struct IcpRecordDev {
    float T[16];            // the iteration's incremental transform
    double mse;
    int pairs, conv_state;
};

}  // namespace ndt
