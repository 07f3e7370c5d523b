/* ndt_hip.h — C-ABI of the MI355X-native NDT scan-matching library (libndt_hip.so).
 *
 * Drop-in boundary for the reference's registration object
 *   pclomp::NormalDistributionsTransform<pcl::PointXYZI, pcl::PointXYZI>
 * (reference: /root/reference/xchu_mapping/include/pclomp/ndt_omp.h:70-497) as used by
 * odom_node (xchu_mapping/src/odom_node.cpp:69-80, 227-228, 277-283, 348-349).
 * Plain C: opaque handle, plain pointers and sizes, status codes — no C++/torch types.
 * One ctx = one HIP device + one HIP stream; a ctx is not thread-safe (same as the reference,
 * which is driven from odom_node's single main thread).
 *
 * Each entry point names the reference interface it replaces.
 */
#ifndef NDT_HIP_H_
#define NDT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Layout version of the structs below and of the buffers the library writes through caller pointers
 * (ndt_result, ndt_pass_record, ndt_pair_desc, ndt_filter_params, ndt_pass_phases' 22 doubles).  History: 1 = round 1;
 * 2 = ndt_result.solver_fallbacks appended, ndt_pass_phases 20 -> 22 doubles; 3 = the Scan Context surface (ndt_sc_params,
 * ndt_sc_result; no earlier layout changed); 4 = the pose-graph surface (ndt_pgo_params, ndt_pgo_result, ndt_pgo_record;
 * no earlier layout changed); 5 = the ISC surface (ndt_isc_params, ndt_isc_result); no earlier layout changed; 6 =
 * ndt_pass_geometry (its 8 ints); no earlier layout changed; ground surface added at 6, size-checked (ndt_ground_params and
 * ndt_ground_result start with their own size, which the library checks; no earlier layout changed); position factors of
 * the pose graph added at 6 (ndt_pgo_add_position, ndt_pgo_get_position_weights: two functions, no struct or buffer layout
 * of their own; no earlier layout changed); ndt_pgo_set_estimate added at 6 (one function, no layout of its own); the
 * pose graph's solver choice added at 6 (ndt_pgo_set_solver, ndt_pgo_get_solver, ndt_pgo_solver_stats with its own
 * ndt_pgo_solver_stats_t; no earlier layout changed).  A caller built against this header checks ndt_abi_version() == NDT_HIP_ABI_VERSION before its first call. */
#define NDT_HIP_ABI_VERSION 6

typedef struct ndt_ctx ndt_ctx;

typedef enum {
    NDT_OK = 0,
    NDT_EINVAL = 1,      /* bad argument                                                         */
    NDT_ENOTARGET = 2,   /* align before setInputTarget (PCL: initCompute fails, align is a no-op) */
    NDT_ENOSOURCE = 3,   /* align before setInputSource                                          */
    NDT_EOVERFLOW = 4,   /* voxel index overflow: grid left empty (VGC applyFilter :79-84 warns)  */
    NDT_EDEVICE = 5,     /* HIP runtime error / no device                                        */
    NDT_ENOMEM = 6
} ndt_status;

/* = pclomp::NeighborSearchMethod order (ndt_omp.h:52-57) */
typedef enum { NDT_KDTREE = 0, NDT_DIRECT26 = 1, NDT_DIRECT7 = 2, NDT_DIRECT1 = 3 } ndt_search;

typedef struct {
    float resolution;                /* setResolution            (ndt_omp.h:127-137)   default 1.0   */
    double step_size;                /* setStepSize              (ndt_omp.h:160-164)   default 0.1   */
    double trans_eps;                /* setTransformationEpsilon (pcl::Registration)   default 0.1   */
    double outlier_ratio;            /* setOulierRatio           (ndt_omp.h:178-182)   default 0.55  */
    int max_iter;                    /* setMaximumIterations     (pcl::Registration)   default 35    */
    int search;                      /* setNeighborhoodSearchMethod (ndt_omp.h:184)    default DIRECT7 */
    int min_points_per_voxel;        /* VGC::setMinPointPerVoxel (voxel_grid_covariance_omp.h:135) default 6 */
    double min_covar_eigvalue_mult;  /* VGC::setCovEigValueInflationRatio (:155)       default 0.01  */
    int precision_mode;              /* 0 = ndt_omp (f32 per pair), 1 = pcl_ndt (f64 per pair, radius),
                                        2 = ndt_cpu (cpu::NormalDistributionsTransform: its own cpu::VoxelGrid
                                        and radius search, f64 per pair; odom_node.cpp:57-68, launch default) */
    int device;                      /* HIP device ordinal                                           */
} ndt_params;

typedef struct {
    float final_tf[16];              /* getFinalTransformation(), column-major (Eigen::Matrix4f)      */
    int nr_iterations;               /* getFinalNumIteration()   (ndt_omp.h:200-204)                 */
    int converged;                   /* hasConverged()                                               */
    double trans_probability;        /* getTransformationProbability() (ndt_omp.h:191-195)           */
    double score;                    /* last computeDerivatives score                                */
    int n_passes;                    /* derivative evaluations performed                             */
    long long n_pairs;               /* total (point, voxel) pairs evaluated over all passes (P)     */
    int solver_fallbacks;            /* Newton solves that took JacobiSVD semantics (degenerate / ill-conditioned H:
                                        kappa_1(H) > 6.25e13 or a zero pivot; ndt_omp_impl.hpp:118-124)   */
} ndt_result;

/* One derivative evaluation: kind 0 = computeDerivatives with Hessian (ndt_omp_impl.hpp:175),
 * 1 = gradient-only MT trial (:869), 2 = computeHessian radius pass (:550). */
typedef struct {
    int kind;
    int newton_iter;
    double x[6];
    double score;
    double g[6];
    double H[36];
    long long pairs;
} ndt_pass_record;

/* Batched offline replay: one independent scan->localmap pair (device-resident float4 xyzw). */
typedef struct {
    const float* d_target_xyz4;
    size_t n_target;
    const float* d_source_xyz4;
    size_t n_source;
    float guess[16];
} ndt_pair_desc;

/* Defaults of the pclomp ctor (ndt_omp_impl.hpp:46-69) + VGC ctor (voxel_grid_covariance_omp.h:202-217). */
ndt_status ndt_default_params(ndt_params* out);

/* new pclomp::NormalDistributionsTransform (odom_node.cpp:71-72) */
ndt_status ndt_create(const ndt_params* params, ndt_ctx** out);
/* setResolution/setStepSize/setTransformationEpsilon/setMaximumIterations/setNeighborhoodSearchMethod
 * (odom_node.cpp:73-78).  Does not rebuild the grid (see ndt_set_target). */
ndt_status ndt_set_params(ndt_ctx* ctx, const ndt_params* params);

/* setInputTarget (ndt_omp.h:117-122 -> init() :271-278 -> VGC::filter(true) :285-297).
 * Copies n points (x,y,z float at the start of each stride_bytes record; 32 = pcl::PointXYZI)
 * and rebuilds the voxel grid on the device.  is_dense = PointCloud::is_dense. */
ndt_status ndt_set_target(ndt_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes, int is_dense);
/* Same, from a device-resident float4 array (no PCIe transfer). */
ndt_status ndt_set_target_device(ndt_ctx* ctx, const float* d_xyz4, size_t n, int is_dense);
/* setInputTarget of n_old + n_new device points whose first n_old are the current target's points (same values, same
 * order) — odom_node's pc_target_ = localmap between localmap resets (odom_node.cpp:233, 349), which only grows by
 * appends.  Same grid as ndt_set_target_device(d_xyz4, n_old + n_new, is_dense) bit for bit; when the current grid's
 * sort is still held (pclomp grid, dense cloud, no other sort on the main stream since, same parameters) it is built by
 * merging the sort of the n_new points into it, otherwise from scratch.  The buffer is referenced like
 * ndt_set_target_device's.  d_new4 (may be NULL): the n_new points are read there and stored at d_xyz4 + 4 * n_old by
 * the build itself, on the ctx stream (the caller's snapshot of a growing map needs no separate copy). */
ndt_status ndt_set_target_append_device(ndt_ctx* ctx, float* d_xyz4, size_t n_old, size_t n_new, int is_dense,
                                        const float* d_new4);

/* cpu::NormalDistributionsTransform::updateVoxelGrid(new_cloud) (ndt_cpu/NormalDistributionsTransform.h:39;
 * odom_node.cpp:344-345): append points to the target (after the existing ones) and update the voxel grid, as if the
 * target had been set to old + new.  Host points (stride as ndt_set_target) or device float4 points (copied). */
ndt_status ndt_update_target(ndt_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes);
ndt_status ndt_update_target_device(ndt_ctx* ctx, const float* d_xyz4, size_t n);

/* setInputSource (pcl::Registration, odom_node.cpp:278). Copies: the host version at once; the device version on the
 * ctx stream with the next align (inside its first kernel) or the next other call that reads the source, whichever
 * comes first — d_xyz4 stays unmodified until then (pcl::Registration keeps the caller's cloud the same way), or until
 * ndt_synchronize. */
ndt_status ndt_set_source(ndt_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes);
ndt_status ndt_set_source_device(ndt_ctx* ctx, const float* d_xyz4, size_t n);

/* align(output, guess) (pcl::Registration::align -> computeTransformation, ndt_omp_impl.hpp:73-164;
 * odom_node.cpp:279).  guess: column-major 4x4.  Synchronous; fills out. */
ndt_status ndt_align(ndt_ctx* ctx, const float guess[16], ndt_result* out);
/* The aligned `output` cloud of align(): source transformed by final_tf, written as x,y,z at each stride. */
ndt_status ndt_get_output(ndt_ctx* ctx, float* xyz, size_t stride_bytes);
/* Per-pass trace of the last align (history of computeDerivatives results). */
ndt_status ndt_get_history(ndt_ctx* ctx, ndt_pass_record* out, int cap, int* n_out);

/* Test hooks: one computeDerivatives pass (ndt_omp_impl.hpp:175) at parameters p with point transform T. */
ndt_status ndt_derivatives(ndt_ctx* ctx, const double p[6], const float T[16], int compute_hessian,
                           double* score, double g[6], double H[36], long long* pairs);
/* computeHessian (radius neighbours, f64; ndt_omp_impl.hpp:550-607) at p with transform T. */
ndt_status ndt_hessian_radius(ndt_ctx* ctx, const double p[6], const float T[16], double H[36], long long* pairs);
/* calculateScore (ndt_omp_impl.hpp:919-952) of the source transformed by T (uses the Gaussian constants the
 * object holds: the constructor's until an align recomputes them, as the reference's members). */
ndt_status ndt_calculate_score(ndt_ctx* ctx, const float T[16], double* out);
/* pcl::Registration::getFitnessScore(max_range) (called by odom_node.cpp:280 after every align): mean of the
 * squared nearest-neighbour distances from the source transformed by T (NULL = the last align's final
 * transformation, identity before any align) to ALL target points, over the distances <= max_range (PCL
 * compares the squared distance); DBL_MAX when none qualifies.  nn_d2 (optional, N floats) receives every
 * point's squared distance. */
ndt_status ndt_fitness_score(ndt_ctx* ctx, const float* T, double max_range, double* out, float* nn_d2);

/* getFitnessScore, asynchronous: enqueued on the ctx's fitness side stream behind everything queued on the ctx
 * stream so far (source, align), so that it runs beside what the caller queues next (a target build, a keyframe
 * insertion); ndt_fitness_score_result waits for it and returns the score (same semantics as ndt_fitness_score). */
ndt_status ndt_fitness_score_async(ndt_ctx* ctx, const float* T, double max_range);
ndt_status ndt_fitness_score_result(ndt_ctx* ctx, double* out);
/* getFitnessScore of an explicit device cloud (float4, n points: normally the source the last align registered) instead
 * of the ctx's source, asynchronous like ndt_fitness_score_async: the cloud is read on the side stream, so the ctx's
 * source may be replaced (the next scan's setInputSource) while the query is in flight; d_src4 stays unmodified until
 * ndt_fitness_score_result. */
ndt_status ndt_fitness_score_async_cloud(ndt_ctx* ctx, const float* T, double max_range, const float* d_src4, size_t n);
/* getFitnessScore of the last align (its final transformation, its target) over a device cloud, asynchronous like
 * ndt_fitness_score_async_cloud, and callable after setInputTarget has replaced the target that align used (odom_node
 * queries at :280 and sets the next target at :349; queuing the query after the new target's build is queued lets that
 * build start first).  The replaced target's index must have been queued (ndt_fitness_index_async after its
 * setInputTarget); NDT_EINVAL otherwise. */
ndt_status ndt_fitness_score_async_aligned(ndt_ctx* ctx, double max_range, const float* d_src4, size_t n);
/* getFitnessScore's nearest-neighbour index over the current target, queued now on the fitness side stream behind the
 * target's points (beside the voxel build and the next align) instead of at the first query after setInputTarget.
 * A scan loop that queries every scan (odom_node.cpp:280) calls it after each setInputTarget.  The index build reads
 * the target cloud: a caller-referenced device target stays unmodified until the next ndt_fitness_score_result or
 * ndt_synchronize. */
ndt_status ndt_fitness_index_async(ndt_ctx* ctx);

/* ---- Point-to-point ICP: pcl::IterativeClosestPoint<PointXYZI, PointXYZI> as pgo_node's PGO::ICPRefine drives it
 * (xchu_mapping/src/pgo_node.cpp:404-483) — a second pcl::Registration operator on the same ctx: it aligns the ctx's
 * current source (setInputSource) to its current target (setInputTarget) and searches the nearest-neighbour index
 * getFitnessScore uses (cell size = the ctx's resolution).  Semantics (PCL 1.7: CorrespondenceEstimation,
 * TransformationEstimationSVD, DefaultConvergenceCriteria; parity unpinned): per iteration the nearest target
 * point of every source point over all target points (FLANN L2_Simple in f32, equal distances to the lowest target
 * index), pairs with d^2 <= max_corr_dist^2 kept, fewer than 3 pairs = NDT_ICP_NO_CORRESPONDENCES; Umeyama estimate
 * without scale (f64 sums and SVD where PCL has f32: documented deviation), applied in f32 to the cloud and to the final
 * transformation; then the criteria in the order of ndt_icp_state, the first that holds ends the align.  These additions
 * left every existing layout as it was. */
typedef enum {
    NDT_ICP_NOT_CONVERGED = 0,
    NDT_ICP_ITERATIONS = 1,          /* iterations >= max_iter                                                      */
    NDT_ICP_TRANSFORM = 2,           /* 0.5 (trace R - 1) >= 1 - trans_eps and |t|^2 <= trans_eps (trans_eps > 0)     */
    NDT_ICP_ABS_MSE = 3,             /* |mse - previous mse| < 1e-12                                                */
    NDT_ICP_REL_MSE = 4,             /* |mse - previous mse| / previous mse < fit_eps (fit_eps > 0)                  */
    NDT_ICP_NO_CORRESPONDENCES = 5   /* fewer than 3 pairs: converged = 0, the final transformation stays as it was  */
} ndt_icp_state;

typedef struct {
    double max_corr_dist;            /* setMaxCorrespondenceDistance   default sqrt(DBL_MAX)   pgo_node: 150        */
    int max_iter;                    /* setMaximumIterations           default 10              pgo_node: 100        */
    double trans_eps;                /* setTransformationEpsilon       default 0 (test off)    pgo_node: 1e-6       */
    double fit_eps;                  /* setEuclideanFitnessEpsilon     default 0 (test off)    pgo_node: 1e-6       */
} ndt_icp_params;

typedef struct {
    float final_tf[16];              /* getFinalTransformation(), column-major                                       */
    int converged;                   /* hasConverged()                                                               */
    int state;                       /* ndt_icp_state of the last iteration                                          */
    int nr_iterations;               /* iterations run (transform estimates applied)                                 */
    double mse;                      /* mean squared pair distance of the last iteration                             */
    long long n_pairs;               /* pairs of the last iteration                                                  */
} ndt_icp_result;

/* One iteration: its incremental transform (identity for a NO_CORRESPONDENCES record), pairs, mse and state. */
typedef struct {
    float T[16];
    long long n_pairs;
    double mse;
    int state;
} ndt_icp_record;

ndt_status ndt_icp_default_params(ndt_icp_params* out);
/* icp.align(output, guess) (pgo_node.cpp:462).  prm NULL = the defaults, guess NULL = identity.  Synchronous. */
ndt_status ndt_icp_align(ndt_ctx* ctx, const ndt_icp_params* prm, const float guess[16], ndt_icp_result* out);
/* Per-iteration trace of the last ICP align. */
ndt_status ndt_icp_history(ndt_ctx* ctx, ndt_icp_record* out, int cap, int* n_out);
/* Test hook: the correspondences of the last iteration run — per source point the matched target index in the caller's
 * order (-1: the pair was rejected by max_corr_dist, or the target is empty) and the squared distance to its nearest
 * target point; *n_out = the source size.  index / d2 may be NULL. */
ndt_status ndt_icp_correspondences(ndt_ctx* ctx, int* index, float* d2, size_t cap, size_t* n_out);
/* After ndt_icp_align, ndt_get_output returns the source transformed by the ICP's final transformation, and
 * ndt_fitness_score with T = NULL scores that transformation (the last align of either kind). */

/* ---- Generalized-ICP: pclomp::GeneralizedIterativeClosestPoint (xchu_mapping/include/pclomp/gicp_omp.h,
 * gicp_omp_impl.hpp), the reference library's third registration method — a pcl::Registration operator on the same ctx
 * as ndt_icp_align.  Semantics are the restatement of DESIGN.md (GICP; parity unpinned): per point of either cloud the
 * covariance of its k nearest neighbours (ascending (d^2, index), the point included), regularised to singular values
 * (1, 1, gicp_epsilon); per outer iteration the exact nearest target point of every source point moved by guess and then
 * by the running transformation, pairs with d^2 < max_corr_dist^2 kept (strict), M_i = (R C1_i R^T + C2_j)^-1; fewer than
 * 4 pairs = NDT_GICP_NO_CORRESPONDENCES; otherwise sum res^T M res / m is minimised over (x, y, z, roll, pitch, yaw) by the
 * project's BFGS with Fletcher's line search (PCL's bfgs.h is not part of the reference tree: documented deviation), and
 * the iteration ends the align when delta < 1 or max_iter is reached.  PCL's treatment of the guess is kept: the
 * objective and the final transformation use R(x) R_guess and t_guess + x_t, the search the full product.
 * k_correspondences above 32, or a cloud with fewer than k points, is NDT_EINVAL (the reference logs and reads an empty
 * vector).  Caller-supplied covariances (setSourceCovariances / setTargetCovariances) are not supported. */
typedef enum {
    NDT_GICP_NOT_CONVERGED = 0,
    NDT_GICP_ITERATIONS = 1,         /* outer iterations >= max_iter                                                 */
    NDT_GICP_DELTA = 2,              /* max |prev - cur| scaled by 1/rot_eps (3x3 corner) or 1/trans_eps is below 1   */
    NDT_GICP_NO_CORRESPONDENCES = 3, /* fewer than 4 pairs: converged = 0, final from the transformation before        */
    NDT_GICP_SOLVER_FAILED = 4       /* the minimiser ran out of evaluations or bracketing steps: as above            */
} ndt_gicp_state;

/* ndt_gicp_record::min_status */
typedef enum {
    NDT_GICP_MIN_RUNNING = 0,
    NDT_GICP_MIN_SUCCESS = 1,        /* |g| < 1e-2                                                                   */
    NDT_GICP_MIN_NO_PROGRESS = 2,    /* no descent direction, or a line search stopped by round-off                  */
    NDT_GICP_MIN_MAX_INNER = 3,      /* max_inner_iter line searches done                                            */
    NDT_GICP_MIN_FAILED = 4
} ndt_gicp_min_status;

typedef struct {
    double max_corr_dist;            /* setMaxCorrespondenceDistance     default 5                                   */
    int max_iter;                    /* setMaximumIterations             default 200                                 */
    double trans_eps;                /* setTransformationEpsilon         default 5e-4                                */
    double rot_eps;                  /* setRotationEpsilon               default 2e-3                                */
    int k_correspondences;           /* setCorrespondenceRandomness      default 20, at most 32                      */
    double gicp_epsilon;             /* smallest singular value of a regularised covariance, default 1e-3            */
    int max_inner_iter;              /* setMaximumOptimizerIterations    default 20                                  */
} ndt_gicp_params;

typedef struct {
    float final_tf[16];              /* getFinalTransformation(), column-major                                       */
    int converged;                   /* hasConverged()                                                               */
    int state;                       /* ndt_gicp_state                                                               */
    int nr_iterations;               /* outer iterations completed                                                   */
    double f;                        /* the objective at the end of the last inner solve                             */
    long long n_pairs;               /* pairs of the last outer iteration                                            */
    long long n_evals;               /* objective evaluations of the whole align                                     */
} ndt_gicp_result;

/* One outer iteration: transformation_ after it (before it for an iteration that ended the align unconverged). */
typedef struct {
    float T[16];
    long long n_pairs;
    double f;
    int inner_iterations;
    int n_evals;
    int min_status;                  /* ndt_gicp_min_status                                                          */
    double delta;
    int state;                       /* ndt_gicp_state                                                               */
} ndt_gicp_record;

ndt_status ndt_gicp_default_params(ndt_gicp_params* out);
/* gicp.align(output, guess) over the ctx's target and source.  prm NULL = the defaults, guess NULL = identity.
 * Synchronous.  Afterwards ndt_get_output and ndt_fitness_score(T = NULL) refer to this align (the last align of any
 * kind).  Covariances are kept until their cloud, k_correspondences or gicp_epsilon changes. */
ndt_status ndt_gicp_align(ndt_ctx* ctx, const ndt_gicp_params* prm, const float guess[16], ndt_gicp_result* out);
/* Per-outer-iteration trace of the last GICP align. */
ndt_status ndt_gicp_history(ndt_ctx* ctx, ndt_gicp_record* out, int cap, int* n_out);
/* Test hooks.  Covariances of the target (which = 0) or source (1) under prm (NULL = defaults), 9 f64 per point; raw != 0:
 * the covariances before the SVD.  *n_out = the cloud's size. */
ndt_status ndt_gicp_covariances(ndt_ctx* ctx, const ndt_gicp_params* prm, int which, int raw, double* out, size_t cap, size_t* n_out);
/* The last outer iteration's pairs: matched target index (-1 rejected), d^2, and M_i (9 f64, rows; rejected: stale). */
/* Both hooks below are NDT_EINVAL once the source has been replaced since that align. */
ndt_status ndt_gicp_correspondences(ndt_ctx* ctx, int* index, float* d2, double* M9, size_t cap, size_t* n_out);
/* The objective of the last outer iteration's pairs and its gradient at x, one launch. */
ndt_status ndt_gicp_evaluate(ndt_ctx* ctx, const double x[6], double* f, double g[6]);
/* Profiling hook (tools/gicp_profile.py): kernel launches and host round trips of the last GICP align. */
ndt_status ndt_gicp_run_stats(ndt_ctx* ctx, int* launches, int* rounds);

/* ---- Scan Context: SCManager (xchu_mapping/include/scancontext/Scancontext.{h,cpp}), pgo_node's default loop detector
 * (loop_method 1: makeAndSaveScancontextAndKeys per keyframe at pgo_node.cpp:236, detectLoopClosureID at :344).  The
 * descriptors (20 rings x 60 sectors over 80 m, lidar height 2.0), their ring keys, sector keys and column norms stay in
 * a database on the device; nothing but the small result record crosses to the host.  Semantics are the restatement of
 * DESIGN.md (parity unpinned): atanf is modelled as the f64 arctangent rounded to f32, Eigen's reductions follow Eigen
 * 3.3's SSE2 order, and of ring keys at an equal distance the lower index is the nearer.  Points with a non-finite
 * coordinate are outside the contract (filter_node removes them) and are skipped.
 * An ndt_sc is created on a ctx, uses that ctx's device and stream, reports its errors through ndt_last_error(ctx), and is
 * destroyed before the ctx. */
typedef struct ndt_sc ndt_sc;

typedef struct {
    double dist_thres;               /* SC_DIST_THRES (setSCdistThres)                 default 0.2                   */
    int num_exclude_recent;          /* NUM_EXCLUDE_RECENT                             default 30                    */
    int num_candidates;              /* NUM_CANDIDATES_FROM_TREE, 1..16                default 3                     */
    int tree_making_period;          /* TREE_MAKING_PERIOD_ (ndt_sc_detect), >= 1      default 30                    */
    double search_ratio;             /* SEARCH_RATIO, 0..1 (1 = all 60 shifts)         default 0.1                   */
} ndt_sc_params;

typedef struct {
    int loop_id;                     /* nn_idx when min_dist < dist_thres, else -1                                   */
    float yaw_diff;                  /* deg2rad(nn_align * 6), narrowed through float as the reference does          */
    double min_dist;                 /* least candidate distance (10000000 when no candidate had one)                */
    int nn_idx, nn_align;            /* its descriptor and column shift                                              */
    int n_candidates;                /* ring-key neighbours compared (0: the early return)                           */
    int cand_idx[16];                /* in ascending ring-key distance; unused slots -1                              */
    double cand_dist[16];            /* distanceBtnScanContext of the query and each candidate                       */
    int cand_shift[16];
} ndt_sc_result;

ndt_status ndt_sc_default_params(ndt_sc_params* out);
ndt_status ndt_sc_create(ndt_ctx* ctx, const ndt_sc_params* prm, ndt_sc** out);   /* prm NULL = the defaults */
void ndt_sc_destroy(ndt_sc* sc);
ndt_status ndt_sc_set_params(ndt_sc* sc, const ndt_sc_params* prm);
/* descriptors stored (-1 for a NULL handle) */
int ndt_sc_size(const ndt_sc* sc);
/* makeAndSaveScancontextAndKeys (:249-260) of a device float4 cloud / of a host cloud (x,y,z at the start of each
 * stride_bytes record); *index (may be NULL) = the slot it took.  n = 0 stores the all-zero descriptor.  Asynchronous on
 * the ctx stream: d_xyz4 stays unmodified until the next synchronising call (ndt_sc_detect, ndt_sc_get, ndt_synchronize). */
ndt_status ndt_sc_add_device(ndt_sc* sc, const float* d_xyz4, size_t n, int* index);
ndt_status ndt_sc_add(ndt_sc* sc, const float* xyz, size_t n, size_t stride_bytes, int* index);
/* saveScancontextAndKeys (:236-246): a ready descriptor, column-major 20 x 60 as Eigen stores it. */
ndt_status ndt_sc_add_descriptor(ndt_sc* sc, const double desc[1200], int* index);
/* detectLoopClosureID (:331-422) for the newest descriptor.  Stateful like the reference: with fewer than
 * num_exclude_recent + 1 descriptors it returns the early record (loop_id -1, yaw_diff 0) and leaves the period counter
 * alone; otherwise the searchable set becomes [0, size - num_exclude_recent) when the counter is a multiple of
 * tree_making_period, the counter advances, and the search runs in the (possibly stale) set. */
ndt_status ndt_sc_detect(ndt_sc* sc, ndt_sc_result* out);
/* Stateless batch form, one launch: query[i] is searched against the ring keys [0, n_search[i]); n_search[i] <= 0 gives
 * the early record. */
ndt_status ndt_sc_detect_batch(ndt_sc* sc, const int* query, const int* n_search, int n, ndt_sc_result* out);
/* distanceBtnScanContext (:116-148) of stored descriptors i and j: the distance and the column shift of j. */
ndt_status ndt_sc_distance(ndt_sc* sc, int i, int j, double* dist, int* shift);
/* Read back slot index: the descriptor (1200 doubles, column-major), ring key (20 floats), sector key (60 doubles); any
 * pointer may be NULL. */
ndt_status ndt_sc_get(ndt_sc* sc, int index, double* desc, float* ringkey, double* sectorkey);

/* ---- Intensity Scan Context: ISCGeneration (xchu_mapping/include/isc/ISCGeneration.{h,cpp}), pgo_node's loop_method 2
 * (makeAndSavedec per keyframe at pgo_node.cpp:239, detectLoopClosureID at :366).  A descriptor is a rings x sectors matrix
 * of bytes (the largest (int)(255 * intensity) of the points of each polar cell, -0.9 <= z <= 30); the database (the
 * descriptors sector-major, per column the ring masks "cell == 0" and "cell == 1", the keyframe positions and travel
 * distances) stays on the device and nothing but the small result record crosses to the host.  Semantics are the
 * restatement of DESIGN.md §2 "ISC" (parity unpinned): atan2f is modelled as the f64 arctangent rounded to f32; three
 * deviations, each where the reference leaves its row or depends on point order: a negative sector index (y = -0, x < 0)
 * is skipped, an intensity outside 0..1 clamps to 0..255 (NaN: 0), and the intensity window wraps its column with a true
 * modulo.  Everything after the binning is integer arithmetic and f64 quotients of integers: bit-exact.
 * An ndt_isc is created on a ctx, uses that ctx's device and stream, reports its errors through ndt_last_error(ctx), and is
 * destroyed before the ctx. */
typedef struct ndt_isc ndt_isc;

typedef struct {
    int rings;                       /* init_param, 1..64                              pgo_node: 60                  */
    int sectors;                     /* init_param, 20..128                            pgo_node: 60                  */
    double max_dis;                  /* init_param, > 0                                pgo_node: 40.0                */
    double skip_neighbour_distance;  /* SKIP_NEIBOUR_DISTANCE                          20.0                          */
    double inflation_covariance;     /* INFLATION_COVARIANCE                           0.03                          */
    double geometry_threshold;       /* GEOMETRY_THRESHOLD                             0.67                          */
    double intensity_threshold;      /* INTENSITY_THRESHOLD                            0.91                          */
    float z_min, z_max;              /* ground_filter's PassThrough limits, inclusive  -0.9, 30.0                    */
} ndt_isc_params;

typedef struct {
    int loop_id;                     /* prev, or -1 (also whenever the winning index is 0, as the reference)         */
    int curr_id;                     /* the query index                                                              */
    int best_id;                     /* the winning index before the "!= 0" rule; 0 when none                        */
    double best_score;               /* geo_score + inten_score of the winner (0 when none)                          */
    double geo_score, inten_score;
    int angle;                       /* the winner's column shift                                                    */
    int n_gated;                     /* pairs that passed the travel / position gate                                 */
    int n_geometry;                  /* of those, past the geometry threshold                                        */
    int n_loop_pairs;                /* of those, past the intensity threshold too                                   */
} ndt_isc_result;

/* pgo_node's init_param values and the five #defines of ISCGeneration.h */
ndt_status ndt_isc_default_params(ndt_isc_params* out);
/* prm NULL = the defaults.  The parameters are fixed at creation: the database layout depends on them. */
ndt_status ndt_isc_create(ndt_ctx* ctx, const ndt_isc_params* prm, ndt_isc** out);
void ndt_isc_destroy(ndt_isc* isc);
/* descriptors stored (-1 for a NULL handle) */
int ndt_isc_size(const ndt_isc* isc);
/* makeAndSavedec (:195-214) of a device float4 x,y,z,intensity cloud / of a host cloud (x,y,z at the start of each
 * stride_bytes record, intensity at float index intensity_offset); pos = the keyframe position as given (pgo_node passes
 * z = 0), narrowed through f32 as pcl::PointXYZI holds it; *index (may be NULL) = the slot it took.  n = 0 stores the
 * all-zero descriptor.  Asynchronous on the ctx stream: d_xyzi4 stays unmodified until the next synchronising call
 * (ndt_isc_detect, ndt_isc_get, ndt_synchronize). */
ndt_status ndt_isc_add_device(ndt_isc* isc, const float* d_xyzi4, size_t n, const double pos[3], int* index);
ndt_status ndt_isc_add(ndt_isc* isc, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset, const double pos[3],
                       int* index);
/* A ready descriptor, row-major rings x sectors bytes. */
ndt_status ndt_isc_add_descriptor(ndt_isc* isc, const unsigned char* bytes, const double pos[3], int* index);
/* detectLoopClosureID (:157-193) for the newest keyframe. */
ndt_status ndt_isc_detect(ndt_isc* isc, ndt_isc_result* out);
/* Stateless batch form, one submission: query[k] is tested as if it were the newest keyframe (only indices <= query[k],
 * with its own travel distance, take part). */
ndt_status ndt_isc_detect_batch(ndt_isc* isc, const int* query, int n, ndt_isc_result* out);
/* is_loop_pair (:216-229) of stored descriptors i (desc1) and j (desc2): the geometry score and its column shift, the
 * intensity score (computed whatever the geometry score is) and the reference's verdict.  Any pointer may be NULL. */
ndt_status ndt_isc_pair(ndt_isc* isc, int i, int j, double* geo, int* angle, double* inten, int* is_loop);
/* calculate_intensity_dis (:259-283) of stored descriptors i and j around a given column shift, 0 <= angle < sectors. */
ndt_status ndt_isc_intensity(ndt_isc* isc, int i, int j, int angle, double* inten);
/* Read back slot index: the descriptor (row-major rings x sectors bytes), the position (3 doubles), the travel distance;
 * any pointer may be NULL. */
ndt_status ndt_isc_get(ndt_isc* isc, int index, unsigned char* bytes, double* pos, double* travel);

/* ---- Pose graph: what pgo_node asks GTSAM for (pgo_node.cpp:249-291 prior and odometry factors, :453-475 loop factors,
 * :498-528 ISAM2Update), solved on the device as a batch problem.  The reference holds no GTSAM source, so this is a model
 * (DESIGN.md "Pose graph", parity unpinned): one SE(3) pose per keyframe in f64, tangent order [wx wy wz vx vy vz],
 * retraction X <- X Exp(d); a prior on node 0 with residual Log(P^-1 X0); between factors with residual
 * e = Log(Z^-1 Xi^-1 Xj) (the full SE(3) logarithm, GTSAM's GTSAM_POSE3_EXPMAP chart) whitened by 1/sqrt(var), and an
 * optional Cauchy kernel (weight k^2 / (k^2 + |e|^2_S), cost k^2/2 log(1 + |e|^2_S / k^2); k = 0: Gaussian); position
 * factors (pgo_node's gtsam::GPSFactor under useGPS, :103-111, :278-287) with residual t_k - z, the translation of X_k less
 * the measured point, whitened and weighted the same way, Jacobian [0 R_k].  The result
 * is a stationary point of the total robust cost, reached by iteratively reweighted Gauss-Newton with exact Jacobians;
 * iSAM2's estimate differs from it by its relinearisation threshold and the order in which loops arrive.
 * Poses and measurements are column-major 4 x 4 doubles (as final_tf is) and must be finite rigid transforms.
 * An ndt_pgo is created on a ctx, uses that ctx's device and stream, reports its errors through ndt_last_error(ctx), and
 * is destroyed before the ctx. */
typedef struct ndt_pgo ndt_pgo;

typedef struct {
    int max_iter;                    /* outer (reweighted Gauss-Newton) iterations, 1..10000   default 200           */
    double step_eps;                 /* stop when max|d| (rad, m) falls below it               default 1e-10         */
    int cg_max_iter;                 /* conjugate-gradient iterations per step, 1..10000       default 500           */
    double cg_rtol;                  /* CG stops at |r| <= cg_rtol |r0| (preconditioned norm)  default 1e-10         */
    double prior_var[6];             /* priorNoise variances (rotation x 3, translation x 3)   default 1e-12 x 6     */
    double odom_var[6];              /* odomNoise variances                                    default 1e-6 x 3, 1e-4 x 3 */
} ndt_pgo_params;

typedef struct {
    int iterations;                  /* steps taken                                                                  */
    int converged;                   /* the last step was below step_eps                                             */
    double cost0, cost;              /* total robust cost at the start / at the returned estimate                    */
    double max_step;                 /* max|d| of the last step                                                      */
    int cg_iterations;               /* summed over the steps                                                        */
} ndt_pgo_result;

typedef struct {
    double cost;                     /* before the step                                                              */
    double max_step;
    int cg_iterations;
} ndt_pgo_record;

ndt_status ndt_pgo_default_params(ndt_pgo_params* out);
ndt_status ndt_pgo_create(ndt_ctx* ctx, const ndt_pgo_params* prm, ndt_pgo** out);   /* prm NULL = the defaults */
void ndt_pgo_destroy(ndt_pgo* pgo);
/* nodes (-1 for a NULL handle) */
int ndt_pgo_size(const ndt_pgo* pgo);
/* A keyframe pose.  Node 0 gets the prior (mean = this pose); every later node gets the odometry edge from its
 * predecessor, measured between the two poses as given (Run(), :249-291).  The pose is also the node's initial estimate. */
ndt_status ndt_pgo_add_node(ndt_pgo* pgo, const double pose[16], int* index);
/* The estimate of a stored node replaced by `pose` (a finite rigid transform, as add_node's).  Host state only: no factor
 * changes and nothing is launched.  For a caller that appends a node whose only new factor is its odometry edge to an
 * optimised graph: the estimate X_{k-1} (P_{k-1}^-1 P_k) makes that edge's residual zero, so a stationary estimate stays
 * stationary and no optimise is needed. */
ndt_status ndt_pgo_set_estimate(ndt_pgo* pgo, int node, const double pose[16]);
/* BetweenFactor(i, j, Z) with diagonal variances and a Cauchy kernel of width robust_k (0: none).  i != j, both stored
 * nodes, either order. */
ndt_status ndt_pgo_add_between(ndt_pgo* pgo, int i, int j, const double Z[16], const double var[6], double robust_k);
/* GPSFactor(node, xyz) with diagonal variances and a Cauchy kernel of width robust_k (0: none).  xyz is in metres in the
 * map frame (pgo_node.cpp:278-287 gives the keyframe's own x and y with variance 1e9 and the altitude less the first fix's
 * with variance 250).  A stored node, finite xyz, finite positive variances; a node may carry any number of them. */
ndt_status ndt_pgo_add_position(ndt_pgo* pgo, int node, const double xyz[3], const double var[3], double robust_k);
/* One optimisation, from the current estimate (a call after more nodes or factors is a warm start, as ISAM2Update is); one
 * launch, synchronises.  A residual rotation within 1e-6 of pi is NDT_EINVAL and a non-finite cost or step NDT_EOVERFLOW;
 * the estimate is then left as it was. */
ndt_status ndt_pgo_optimize(ndt_pgo* pgo, ndt_pgo_result* out);
/* The current estimate: min(cap, size) column-major poses; *n_out (may be NULL) = size. */
ndt_status ndt_pgo_get_poses(ndt_pgo* pgo, double* poses16, int cap, int* n_out);
/* The robust weight of every between factor the last optimise held, at its returned estimate, in insertion order. */
ndt_status ndt_pgo_get_weights(ndt_pgo* pgo, double* w, int cap, int* n_out);
/* The robust weight of every position factor the last optimise held, in insertion order. */
ndt_status ndt_pgo_get_position_weights(ndt_pgo* pgo, double* w, int cap, int* n_out);
/* One record per step of the last optimise. */
ndt_status ndt_pgo_history(ndt_pgo* pgo, ndt_pgo_record* out, int cap, int* n_out);

/* The linear solver of each Gauss-Newton step.  CG (the default): conjugate gradients inside the one launch.  DIRECT: the
 * rank-d part of the normal equations (d = 6 x between factors + 3 x position factors) is factorised exactly as a dense
 * d x d matrix, a fixed sequence of launches per step; same inputs, same warm start, max_iter and step_eps, same errors,
 * weights and history; cg_iterations is 0 in the result and in every record, cg_max_iter and cg_rtol are ignored.  A DIRECT
 * optimise with d > 8192 is NDT_EINVAL and leaves the estimate unchanged. */
#define NDT_PGO_SOLVER_CG 0
#define NDT_PGO_SOLVER_DIRECT 1
typedef struct {
    int solver;                      /* the solver the last optimise used                                            */
    int d;                           /* 6 m + 3 np of that graph                                                     */
    int tile;                        /* DIRECT: tile width of the blocked factorisation (CG: 0)                      */
    int factorizations;              /* DIRECT: factorisations run, one per step                                     */
    int refined;                     /* DIRECT: 1 when a refinement pass ran after each solve                        */
} ndt_pgo_solver_stats_t;
/* Host state only: the solver of later optimises.  An unknown value is NDT_EINVAL. */
ndt_status ndt_pgo_set_solver(ndt_pgo* pgo, int solver);
int ndt_pgo_get_solver(const ndt_pgo* pgo);              /* -1 for a NULL handle */
/* Of the last optimise whose launches ran, whether it returned NDT_OK or found a rotation at pi or a non-finite value (all
 * zero before the first; an optimise refused before its launches, or ended by a device error, leaves them as they were). */
ndt_status ndt_pgo_solver_stats(ndt_pgo* pgo, ndt_pgo_solver_stats_t* out);

/* ---- Global map: what pgo_node builds three times from its keyframes and their current poses (pgo_node.cpp) — SaveMap
 * (:620-653, every keyframe, finalMap.pcd), PublishPoseAndFrame (:744-812, every second keyframe, again as the graph
 * changes) and LoopFindNearKeyframesCloud (:530-554, root +- 25): each keyframe moved by its pose
 * (pcl::transformPointCloud, f32), stacked, pcl::VoxelGrid(leaf).  The keyframes live on the device once, in one
 * growing arena of float4 x,y,z,intensity points; a build stacks any selection of them in one launch and filters it
 * with the ctx's VoxelGrid (the restatement of DESIGN.md §2; the stacked cloud equals per-keyframe ndt_transform_device
 * bit for bit, the map equals ndt_voxel_downsample_device of it).  Non-finite coordinates are outside the contract
 * (filter_node removes them upstream).
 * An ndt_map is created on a ctx, uses that ctx's device and stream, reports its errors through ndt_last_error(ctx), and
 * is destroyed before the ctx. */
typedef struct ndt_map ndt_map;

ndt_status ndt_map_create(ndt_ctx* ctx, ndt_map** out);
void ndt_map_destroy(ndt_map* m);
/* keyframes stored (-1 for a NULL handle) */
int ndt_map_size(const ndt_map* m);
/* points held / points the arena has room for (64-bit counts, so through a pointer like every other wide result here) */
ndt_status ndt_map_points(const ndt_map* m, long long* points);
ndt_status ndt_map_capacity(const ndt_map* m, long long* points);
/* Room for at least `points` points.  The arena also grows by itself, to at least twice its size, the held points
 * moved device to device on the ctx stream: keyframe contents survive bit for bit, pointers from ndt_map_keyframe do
 * not.  A growth that fails (NDT_ENOMEM) leaves the store as it was. */
ndt_status ndt_map_reserve(ndt_map* m, long long points);
/* A keyframe from a host cloud (x,y,z at the start of each stride_bytes record, intensity at float index
 * intensity_offset; synchronises) / from a device float4 cloud (device-to-device copy on the ctx stream, no transfer;
 * asynchronous: d_xyzi4 stays unmodified until the next synchronising call).  *index (may be NULL) = the slot it took.
 * n = 0 is legal: an empty keyframe keeps its index. */
ndt_status ndt_map_add(ndt_map* m, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset, int* index);
ndt_status ndt_map_add_device(ndt_map* m, const float* d_xyzi4, size_t n, int* index);
/* The stored keyframe on the device (valid until the next ndt_map_add[_device] / ndt_map_reserve; it can feed
 * ndt_sc_add_device, ndt_isc_add_device, ndt_set_source_device ...) / copied to the host: out4 receives min(cap, n)
 * points, *n_out (may be NULL) = n. */
ndt_status ndt_map_keyframe(ndt_map* m, int index, const float** d_xyzi4, size_t* n);
ndt_status ndt_map_get_keyframe(ndt_map* m, int index, float* out4, size_t cap, size_t* n_out);
/* Points of a selection (what a caller buffer for ndt_map_build must hold): index[0..n_sel), NULL = 0..n_sel-1. */
ndt_status ndt_map_count(ndt_map* m, const int* index, int n_sel, long long* total);
/* Stack keyframes index[0..n_sel) (NULL = 0..n_sel-1), keyframe k moved by the column-major 4x4 float T16 + 16*k, in
 * selection order, then pcl::VoxelGrid(leaf); leaf == 0: the stacked cloud itself.  d_out4 NULL: the map's own result
 * buffer (valid until the next build); else a caller buffer with room for cap >= total points (total = ndt_map_count).
 * *n_out = the points written.  A repeated index is stacked twice.  NDT_EINVAL: an index outside the store, a total
 * above 2^31 - 1 points, cap < total, T16 NULL with n_sel > 0.  An empty selection or one of 0 points: NDT_OK, *n_out =
 * 0.  NDT_EOVERFLOW: the leaf is too small for pcl::VoxelGrid's index range; the result is the stacked cloud, as
 * pcl::VoxelGrid outputs its input then.  One k_map_stack launch whatever n_sel is; synchronises. */
ndt_status ndt_map_build(ndt_map* m, const int* index, const float* T16, int n_sel, float leaf, float* d_out4, size_t cap,
                         size_t* n_out);
/* The last build into the map's own buffer, on the device / copied to the host (min(cap, n) points, *n_out = n).  A
 * build into a caller buffer leaves it as it was; NDT_EINVAL before the first such build. */
ndt_status ndt_map_result(ndt_map* m, const float** d_out4, size_t* n);
ndt_status ndt_map_get(ndt_map* m, float* out4, size_t cap, size_t* n_out);
/* The last build's launch (a test hook): out[0] workgroups (0: nothing to stack), out[1] threads per workgroup, out[2]
 * output points a workgroup takes at a time, out[3] segments (= n_sel). */
ndt_status ndt_map_geometry(ndt_map* m, int out[4]);

/* Voxel grid inspection: header = min_b[3], max_b[3], div_b[3], divb_mul[3], n_leaves, n_cloud, overflow,
 * n_valid (16 ints).  Leaves with >= min points (the reference's KD cloud) in ascending key order. */
ndt_status ndt_grid_info(ndt_ctx* ctx, int header[16]);
ndt_status ndt_grid_leaves(ndt_ctx* ctx, int* keys, int* npts, double* mean, double* icov9, float* centroid3,
                           int cap, int* n_out);

/* Pass-chain options, tuning and test hooks (defaults = the measured best; the results of every combination agree with
 * the oracle within the parity bars): lead_tail 1 runs an align whose passes are latency-bound (direct search, no
 * More-Thuente loop, < 256 Ki source points, not inside ndt_align_batch) as a leading-tail chain — each pass's Newton
 * step at the start of the next pass kernel — and 0 keeps last-workgroup tails everywhere (bitwise the same records;
 * tests/test_gpu_lead.py); points_per_thread 2 lets large last-workgroup-tail passes hold two points per thread per tile,
 * 1 keeps one (another fixed f64 summation order), 3 runs them as a grid of one-tile workgroups (one 256-point tile
 * each, three waves per SIMD, partials summed in two levels: another fixed order); source_order 1 visits clouds of >= 256 Ki points in
 * target-cell order during an align, 0 keeps the caller's order (another fixed f64 summation order).  Applies to the
 * ctx and its batch helper contexts; no align may be in flight. */
ndt_status ndt_set_pass_options(ndt_ctx* ctx, int lead_tail, int points_per_thread, int source_order);

/* The launch geometry of a derivative-pass kernel for the ctx's current source, target, parameters and pass options
 * (a test hook: the thresholds between the geometries depend on the device's CU count).  which: 0 = k_pass_direct (the
 * last-workgroup-tail direct pass), 1 = k_pass_lead (the leading-tail direct pass), 2 = k_pass_radius.  out[0]
 * workgroups, out[1] threads per workgroup, out[2] points per workgroup and tile, out[3] points per thread, out[4] 1 =
 * the one-tile kernel, out[5] tiles per workgroup, out[6] groups of the two-level partial hand-off (0 = one level),
 * out[7] workgroups per group (0 = one level).  Computed by the functions the launchers use; launches nothing. */
ndt_status ndt_pass_geometry(ndt_ctx* ctx, int which, int out[8]);

/* Target-build robustness hooks (no reference counterpart).  A target sort whose decoupled look-back timed
 * out (a predecessor tile never became resident: blockIdx.x tile order relies on each XCD dispatching its workgroups in
 * order, which heavy concurrent work on other streams can defeat), whose key needed more radix passes than were
 * launched (the count is predicted from the previous grid), or whose merge-extended sort could not be exact, is flagged
 * on the device and re-run from scratch by the align (or the next synchronous grid reader) — with tiles taken by atomic
 * ticket from then on after a timeout.  ndt_set_build_options (test hook): tile_tickets 1 = tiles by atomic ticket
 * always, 0 = by workgroup index (default); radix_passes 1..4 = launch exactly that many radix passes per target sort
 * (too few is flagged and re-run with four), 0 = predicted (default).  ndt_build_stats: out[0] full builds, out[1]
 * merge-extended builds, out[2] builds re-run after a flag, out[3] of those the look-back timeouts, out[4] contexts whose
 * tiles are taken by ticket, out[5] radix passes the next target sort launches; [0..4] include ndt_align_batch's helper
 * contexts. */
ndt_status ndt_set_build_options(ndt_ctx* ctx, int tile_tickets, int radix_passes);
ndt_status ndt_build_stats(ndt_ctx* ctx, long long out[6]);

/* align split in two: ndt_align_async queues the registration on the ctx stream and returns; ndt_align_wait waits for it
 * and fills out (same result as ndt_align).  One align in flight per ctx; several ctxs (streams) run concurrently. */
ndt_status ndt_align_async(ndt_ctx* ctx, const float guess[16]);
ndt_status ndt_align_wait(ndt_ctx* ctx, ndt_result* out);

/* Batched offline alignment of independent pairs on this ctx's device: pairs round-robin over three
 * streams (this ctx and two helper ctxs, created on first use), one registration in flight per stream; per-pair results
 * bit-identical to one-by-one aligns. */
ndt_status ndt_align_batch(ndt_ctx* ctx, const ndt_pair_desc* pairs, int n_pairs, ndt_result* out);

/* pcl::VoxelGrid<PointXYZI> downsample (odom_node.cpp:96-99, 334-335): per-voxel mean of x,y,z,intensity,
 * output ordered by ascending voxel index.  out4 receives x,y,z,intensity per output point. */
ndt_status ndt_voxel_downsample(ndt_ctx* ctx, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset,
                                float leaf, float* out4, size_t cap, size_t* n_out);

/* filter_node front end (xchu_mapping/src/filter_node.cpp:218-273): the cloud odom_node receives on
 * /filtered_points.  removeNaNFromPointCloud (non-finite points dropped) -> keep r_min < sqrt(x^2+y^2) < r_max (double)
 * -> pcl::VoxelGrid<PointXYZI>(leaf) -> pcl::StatisticalOutlierRemoval(mean_k, stddev_mul) (use_outlier_removal_method,
 * filter_node.h:71).  Output x,y,z,intensity in the reference's order (voxel index order, outliers removed). */
typedef struct {
    float leaf;          /* downSizeFilterKeyFrames leaf size   (filter_node.cpp:33-34)  default 0.5  */
    double r_min, r_max; /* range crop on sqrt(x^2+y^2)          (:239-247)               default 1, 60 */
    int mean_k;          /* StatisticalOutlierRemoval::setMeanK  (:256-259)               default 30 (<= 63) */
    double stddev_mul;   /* setStddevMulThresh                   (:257-260)               default 1.0  */
    int outlier_method;  /* use_outlier_removal_method (filter_node.h:71): 0 = StatisticalOutlierRemoval (default),
                            1 = RadiusOutlierRemoval (:265-272)                                             */
    double ror_radius;   /* RadiusOutlierRemoval::setRadiusSearch          default 0.8              */
    int ror_min_neighbors; /* setMinNeighborsInRadius (neighbours counted with the point itself) default 5 */
} ndt_filter_params;
ndt_status ndt_filter_default_params(ndt_filter_params* out);
/* host cloud: x,y,z at the start of each stride_bytes record, intensity at float index intensity_offset; out4 receives
 * up to cap points (x,y,z,i); *n_out = the filtered size.  A cloud left with <= mean_k points after the voxel filter is
 * returned without outlier removal (PCL reads past its neighbour list there). */
ndt_status ndt_filter_scan(ndt_ctx* ctx, const ndt_filter_params* prm, const float* xyzi, size_t n, size_t stride_bytes,
                           int intensity_offset, float* out4, size_t cap, size_t* n_out);
/* device float4 (x,y,z,i) in and out (d_out4 capacity n, must not alias d_in4); synchronises. */
ndt_status ndt_filter_scan_device(ndt_ctx* ctx, const ndt_filter_params* prm, const float* d_in4, size_t n, float* d_out4, size_t* n_out);
/* per-point SOR distances and threshold of the last filter_scan (test hook): dist[0..n_voxel) in voxel order,
 * thr = {threshold, mean, stddev}; *n_voxel = points after the voxel filter. */
ndt_status ndt_filter_last_stats(ndt_ctx* ctx, float* dist, size_t cap, size_t* n_voxel, double thr[3]);

/* filter_node's ground detection (xchu_mapping/src/filter_node.cpp:53-216: DetectPlane with PlaneClip and
 * NormalFiltering; defaults filter_node.h:62-71): the floor coefficients of /ground_coeffs and the /normal_ground_points,
 * /ground_points and /no_ground_points clouds.  tilt -> height clip (two PlaneClipper3D calls) -> normal filter (k nearest
 * neighbours within the clipped cloud, normal flipped to the viewpoint (0,0,sensor_height), |n.z| against
 * normal_filter_thresh) -> tilt back -> pcl::RandomSampleConsensus over SampleConsensusModelPlane (the model's
 * boost::mt19937 seeded 12345 per scan) -> the gates on the inlier count and on the floor's normal.  PCL is not part of
 * the reference tree: the semantics are the restatement of DESIGN.md §2 "Ground" (parity with PCL unpinned).
 * Both structs start with their own size: the caller sets struct_size = sizeof(its struct) before any call that takes
 * one, and the library answers NDT_EINVAL when that is not the size it was built with. */
typedef enum {
    NDT_GROUND_OK = 0,
    NDT_GROUND_TOO_FEW_POINTS = 1,   /* fewer than floor_pts_thresh points after the normal filter (:144)  */
    NDT_GROUND_TOO_FEW_INLIERS = 2,  /* fewer than floor_pts_thresh inliers, or no model at all (:158)       */
    NDT_GROUND_NOT_VERTICAL = 3      /* the floor's normal is further than floor_normal_thresh from vertical (:169) */
} ndt_ground_reason;
typedef enum { NDT_GROUND_CLOUD_NORMAL = 0, NDT_GROUND_CLOUD_GROUND = 1, NDT_GROUND_CLOUD_NO_GROUND = 2 } ndt_ground_cloud_kind;

typedef struct {
    uint32_t struct_size;        /* sizeof(ndt_ground_params), set by the caller                                  */
    double tilt_deg;             /* filter_node.h:63   default 0                                                    */
    double sensor_height;        /* :64                default 2.0                                                  */
    double height_clip_range;    /* :65                default 2.5 (keeps -4.5 <= z < 0.5 with the defaults)        */
    int floor_pts_thresh;        /* :67                default 512 (>= 3)                                           */
    double floor_normal_thresh;  /* :68  degrees       default 10                                                   */
    int use_normal_filtering;    /* :69                default 1                                                    */
    double normal_filter_thresh; /* :70  degrees       default 20                                                   */
    int normal_k;                /* NormalEstimation::setKSearch (filter_node.cpp:81)  default 10 (1..20)           */
    double ransac_threshold;     /* setDistanceThreshold (:151)                        default 0.1                  */
    double ransac_probability;   /* pcl::SampleConsensus probability_                  default 0.99                 */
    int ransac_max_iterations;   /* pcl::SampleConsensus max_iterations_               default 1000 (1..4000)       */
    int literal_no_ground;       /* 0 (default): /no_ground_points is the input without the points the inliers came
                                    from; 1: the reference's form (:197-202), which removes the input points whose
                                    index equals an inlier's index in the filtered cloud                            */
    float cloud_leaf;            /* downSizeNoGroundFrames leaf (:36) applied by ndt_ground_cloud, default 0.2; 0 = raw */
} ndt_ground_params;

typedef struct {
    uint32_t struct_size;        /* sizeof(ndt_ground_result), set by the caller                                  */
    int found;                   /* 0: the reference returns Vector4f::Identity() (see reason)                     */
    float coeffs[4];             /* a, b, c, d of the floor (normal upward); zeros when not found                   */
    int n_input, n_clipped, n_normal, n_inliers;  /* points: in, after the clip, after the normal filter, inliers   */
    int iterations, skipped;     /* RandomSampleConsensus iterations_ and its skipped (degenerate) samples          */
    int winner[3];               /* the winning sample as indices into the input cloud (-1 without a model)         */
    int reason;                  /* ndt_ground_reason                                                               */
    int stream_fallbacks;        /* times the scan's sampler ran past the uploaded generator table and the host
                                    continued the stream                                                            */
    double k;                    /* the loop's last bound on the iterations                                         */
} ndt_ground_result;

ndt_status ndt_ground_default_params(ndt_ground_params* out);
/* host cloud (as ndt_filter_scan's) -> the floor; synchronises.  The clouds stay on the device until the next detect. */
ndt_status ndt_ground_detect(ndt_ctx* ctx, const ndt_ground_params* prm, const float* xyzi, size_t n, size_t stride_bytes,
                             int intensity_offset, ndt_ground_result* result);
/* device float4 (x,y,z,i) cloud; it is copied, so the caller may reuse the buffer after the call. */
ndt_status ndt_ground_detect_device(ndt_ctx* ctx, const ndt_ground_params* prm, const float* d_in4, size_t n, ndt_ground_result* result);
/* One cloud of the last detect (ndt_ground_cloud_kind), passed through pcl::VoxelGrid(cloud_leaf) unless the leaf is 0:
 * up to cap points (x,y,z,i) to out4, *n_out = the cloud's size.  The ground and no-ground clouds are empty when no floor
 * was found (the reference publishes neither then). */
ndt_status ndt_ground_cloud(ndt_ctx* ctx, int which, float* out4, size_t cap, size_t* n_out);
/* the same into device memory (d_out4: capacity n_input points) */
ndt_status ndt_ground_cloud_device(ndt_ctx* ctx, int which, float* d_out4, size_t cap, size_t* n_out);
/* CloudFilter::Run (filter_node.cpp:218-273 + DetectPlane): ndt_filter_scan_device, then the detect over its output
 * without a host copy of the cloud in between.  d_out4 / *n_out: the filtered scan, as ndt_filter_scan_device's. */
ndt_status ndt_filter_ground_scan(ndt_ctx* ctx, const ndt_filter_params* fprm, const ndt_ground_params* gprm, const float* d_in4,
                                  size_t n, float* d_out4, size_t* n_out, ndt_ground_result* result);
/* hypotheses scored per launch of the plane scoring kernel (the B of DESIGN.md §2 "Ground") */
int ndt_ground_batch(void);
/* Test hooks.  Per point of the clipped cloud of the last detect: normal4 = the oriented normal and |n.z| of the
 * normalised normal (zeros without normal filtering), keep = the filter's flag, origin = its index in the input cloud,
 * nbr = its normal_k neighbours (indices into the clipped cloud, ascending (d2, index), -1 past the cloud's size);
 * any pointer may be NULL; *n_out = the clipped cloud's size. */
ndt_status ndt_ground_last_normals(ndt_ctx* ctx, float* normal4, int* keep, int* origin, int* nbr, size_t cap, size_t* n_out);
/* Every hypothesis the last detect's loop looked at, in order: its sample (indices into the cloud after the normal
 * filter), its coefficients before the sign is settled, its inlier count and its status (1 scored, 0 degenerate sample). */
ndt_status ndt_ground_last_hypotheses(ndt_ctx* ctx, int* triples, float* coeffs, int* counts, int* status, size_t cap, size_t* n_out);
/* The next detects take these n_triples samples in place of the sampler's (the loop ends where the list does);
 * n_triples = 0 restores the sampler.  Indices outside the cloud after the normal filter end the list early. */
ndt_status ndt_ground_set_samples(ndt_ctx* ctx, const int* triples, size_t n_triples);

/* Device-resident variants used by the odom_node replay driver (include/ndt_odom.h), all ordered on the ctx's
 * stream.  d_in4/d_out4 are float4 x,y,z,intensity arrays.
 * pcl::transformPointCloud(in, out, T) (odom_node.cpp:220, 290): out may equal in; asynchronous. */
ndt_status ndt_transform_device(ndt_ctx* ctx, const float T[16], const float* d_in4, size_t n, float* d_out4);
/* pcl::VoxelGrid<PointXYZI>::filter (odom_node.cpp:334-335) of a device cloud: d_out4 (capacity n, must not
 * alias d_in4) receives the voxel means in ascending voxel order; *n_out their count (synchronises). */
ndt_status ndt_voxel_downsample_device(ndt_ctx* ctx, const float* d_in4, size_t n, float leaf, float* d_out4, size_t* n_out);
/* odom_node keyframe insertion (odom_node.cpp:290, 333-338), asynchronous: transformPointCloud(scan, T) ->
 * VoxelGrid(leaf) -> the voxel means appended at d_map_a + n_a and d_map_b + n_b (localmap and tmp_map; float4
 * clouds with room for n more points each), queued on the ctx's insertion side stream behind everything queued on
 * the ctx stream so far (it runs beside what the caller queues next, e.g. the next target build); the scan and the two
 * appended ranges stay untouched until ndt_keyframe_insert_result, which waits and returns how many points were
 * appended (NDT_EOVERFLOW when the leaf overflowed the index range: the transformed scan itself was appended, as
 * pcl::VoxelGrid outputs its input then). */
ndt_status ndt_keyframe_insert_async(ndt_ctx* ctx, const float T[16], const float* d_scan4, size_t n, float leaf, float* d_map_a,
                                     size_t n_a, float* d_map_b, size_t n_b);
ndt_status ndt_keyframe_insert_result(ndt_ctx* ctx, size_t* n_inserted);
/* Marks the point on the ctx stream that the next ndt_fitness_score_async[_cloud] and the next
 * ndt_keyframe_insert_async queue behind (instead of "everything queued so far" at their own calls), so that a scan
 * loop can queue its target copy and build on the ctx stream first and post the side-lane jobs after them, beside
 * them.  A mark not taken by the next align is dropped. */
ndt_status ndt_side_lanes_mark(ndt_ctx* ctx);
/* Device-to-device copy, asynchronous on the ctx stream. */
ndt_status ndt_memcpy_d2d(ndt_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);

/* Device memory helpers (callers without their own GPU runtime binding, e.g. the bench). */
ndt_status ndt_device_alloc(ndt_ctx* ctx, size_t bytes, void** d_ptr);
ndt_status ndt_device_free(ndt_ctx* ctx, void* d_ptr);
ndt_status ndt_memcpy_h2d(ndt_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
ndt_status ndt_memcpy_d2h(ndt_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
/* Waits for the ctx stream and its side streams (getFitnessScore, keyframe insertion). */
ndt_status ndt_synchronize(ndt_ctx* ctx);

/* Timing of the last set_target / align on the device (the 100 MHz device clock, s_memrealtime; ms) and the dominant
 * kernel's average duration (derivative pass, ms) with its algorithmic bytes per launch. */
ndt_status ndt_last_timings(ndt_ctx* ctx, double* ms_build, double* ms_align, double* ms_pass_avg, double* pass_bytes_avg);
/* Profiling breakdown of the average derivative pass (ms), from in-kernel stamps; the 22 columns are named, in order, by
 * kPhaseNames of csrc/ndt_stamps.h, which also holds the stamp slots and the phase sequences: [0] workgroup bodies
 * (first start .. last workgroup's partials stored), [1] hand-off (ticket + acquire), [2] last workgroup's
 * fixed-order partials reduction, [3] AlignState staged into LDS, [4] Newton/More-Thuente control step,
 * [5] next transform + angle tables, [6] state write-back and drain; [7..11] (profiling build
 * libndt_hip_dbg.so only, else 0) mean workgroup entry after the first, probes, pair compaction, pair math,
 * block reduction; [12..19] (profiling build) history record + state copy, state machine, solve set-up,
 * the 6x6 solve, after it, sin/cos of the next angles, transform + table rows, table write-back; [20..21]
 * (profiling build) start of the speculative Newton solve after staging, its duration.
 * Profiling aid, no reference counterpart. */
ndt_status ndt_pass_phases(ndt_ctx* ctx, double ms[22]);
/* Enable/disable the in-kernel per-pass timing stamps (s_memrealtime). */
ndt_status ndt_set_profiling(ndt_ctx* ctx, int enable);

const char* ndt_last_error(const ndt_ctx* ctx);
/* NDT_HIP_ABI_VERSION the library was built with */
int ndt_abi_version(void);
void ndt_destroy(ndt_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* NDT_HIP_H_ */
