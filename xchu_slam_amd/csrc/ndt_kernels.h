// ndt_kernels.h — the one declaration of every kernel of the library (and of the profiling build's dbg_read_blk).
// Included by the kernel units that define them and by the host units that launch them: a declaration that drifts
// from its definition is then an overload nothing defines, and the library's link (--no-undefined) fails.
#pragma once
#include <hip/hip_runtime.h>
#include "ndt_types.h"
#include "ndt_linalg.h"
#include "ndt_icp.h"
#include "ndt_gicp.h"
#include "ndt_sc.h"
#include "ndt_isc.h"
#include "ndt_pgo.h"
#include "ndt_map.h"
#include "ndt_ground.h"

namespace ndt {
__global__ void k_minmax(const float4*, int, int, float*, int*, unsigned long long*, const GridHeader*, GridHeader*, float4*);
__global__ void k_keys(const float4*, int, int, const float*, int, GridHeader*, float, int, double, int, int, int*, int*, int*, unsigned*, int,
                       int*, long long, int2*, long long, const GridHeader*, int);
__global__ void k_merge_append(int*, int*, int*, int*, const GridHeader*, int, const int*, const int*, const int*, const int*, int,
                               GridHeader*, const float4*);
template <int ITEMS>
__global__ void k_radix_onesweep(int*, int*, int*, int*, int, int, const GridHeader*, int*, unsigned*, int, GridHeader*, int, int);
__global__ void k_scan_onepass(const int*, int, const int*, int*, int*, ScanCtx, GridHeader*);
__global__ void k_seg_scan(const int*, const int*, int, GridHeader*, int*, ScanCtx);
__global__ void k_cloud_scan(const int*, int, GridHeader*, int2*, ScanCtx, unsigned);

template <int WAVES>
__global__ void k_leaf_finalize(const float4*, const int*, const int*, const int*, const int*, const int2*, GridHeader*,
                                VoxelRec*, float4*, double*, int*, double*, int*, int2*, int*);
__global__ void k_sorted_gather(const float4*, const int*, const int*, const GridHeader*, float4*, int);
__global__ void k_src_keys(const float4*, int, Mat4f, const GridHeader*, int*, int*, int*, unsigned*, int);
__global__ void k_src_gather(const float4*, const int*, const int*, const GridHeader*, float4*, int);
__global__ void k_crop_flags(const float4*, int, double, double, int*);
__global__ void k_compact4(const float4*, const int*, const int*, int, float4*);
template <int C>
__global__ void k_sor_knn(const float4*, int, int, const GridHeader*, const int*, const int*, const float4*, float*);
__global__ void k_sor_stats(const float*, int, double, double*);
__global__ void k_sor_keep(const float*, int, const double*, int*);
__global__ void k_ror_keep(const float4*, int, double, int, const GridHeader*, const int*, const int*, const float4*, int*);
__global__ void k_ground_clip_flags(const float4*, int, float, float, int*);
__global__ void k_ground_origin(const int*, const int*, const int*, int, int*);
template <int C>
__global__ void k_ground_normals(const float4*, int, int, int, float, double, const GridHeader*, const int*, const int*, const float4*,
                                 const int*, float4*, int*, int*);
__global__ void k_ground_sample(const float4*, GroundState*, int, const unsigned*, int2*, int4*);
__global__ void k_ground_score(const float4*, GroundState*, int, const int4*, float4*, int*, int*, double*, unsigned*);
__global__ void k_ground_finish(const float4*, const int*, int, GroundState*, const int4*, const float4*, int*, int*);
__global__ void k_ground_unmarked(const int*, int, int*);
__global__ void k_downsample_finalize(const float4*, const int*, const GridHeader*, float4*);
__global__ void k_fit_gather(const float4*, const int*, const int*, const int*, const int*, const int*, int, const GridHeader*, float4*,
                             int*, int*, int*);
__global__ void k_icp_pass(float4*, int, IcpState*, const GridHeader*, const int*, const int*, const float4*, const int*, int*, float*,
                           double*, unsigned*, IcpRecordDev*);
template <int C>
__global__ void k_gicp_cov(const float4*, int, int, double, const GridHeader*, const int*, const int*, const float4*, const int*, double*,
                           double*);
__global__ void k_gicp_pairs(const float4*, int, GicpState*, const GridHeader*, const int*, const int*, const float4*, const int*,
                             const double*, const double*, int*, float*, float4*, float4*, double*, unsigned*, GicpRecordDev*);
__global__ void k_gicp_eval(const float4*, int, GicpState*, const int*, const float4*, const float4*, const double*, double*, unsigned*,
                            GicpRecordDev*);
__global__ void k_sc_make(const float4*, int, unsigned*);
__global__ void k_sc_finalize(const unsigned*, ScDb, int);
__global__ void k_sc_detect(ScDb, const int*, const int*, int, int, ScDetectArgs, ndt_sc_result*);
__global__ void k_isc_make(const float4*, int, IscGeom, unsigned*);
__global__ void k_isc_finalize(const unsigned*, IscDb, int, int, int, double, double, double, double);
__global__ void k_isc_detect(IscDb, const int*, int, IscDetectArgs, IscPartial*);
__global__ void k_isc_reduce(const IscPartial*, const int*, int, int, IscDetectArgs, ndt_isc_result*);
__global__ void k_pgo_optimize(PgoGraph, PgoArgs);
__global__ void k_pgo_direct_step(PgoGraph, PgoArgs, PgoDirect, int);
__global__ void k_pgo_schur(PgoGraph, PgoDirect);
__global__ void k_pgo_chol_diag(PgoDirect, int);
__global__ void k_pgo_chol_panel(PgoDirect, int);
__global__ void k_pgo_chol_trail(PgoDirect, int);
__global__ void k_pgo_chol_back(PgoDirect);
__global__ void k_map_stack(const float4*, const int*, const long long*, const Mat4f*, int, int, int, float4*);
__global__ void k_fit_block_flags(const int*, const GridHeader*, int*);
__global__ void k_append2(const float4*, const float4*, int, const GridHeader*, float4*, float4*);
__global__ void k_fit_block_clear(int*, const GridHeader*);
__global__ void k_fit_tables(const int*, const int*, const int*, const int*, const GridHeader*, int*, int*);
__global__ void k_fitness(const float4*, int, Mat4f, const GridHeader*, const int*, const int*, const float4*, double, float*, double*,
                          int*, unsigned*, double*, long long*);
__global__ void k_score_radius(const float4*, int, Mat4f, const GridHeader*, const int2*, const int*, const VoxelRec*, const float4*,
                               const double*, double, double, double, float, double*);
template <int SEARCH, int PPT, bool ONE_TILE>
__global__ void k_pass_direct(const float4*, int, int, const GridHeader*, const int2*, const int*, const VoxelRec*, const AlignState*,
                              AlignState*, double*, unsigned*, double*, PassRecordDev*, int, int, unsigned long long*, int4*);
__global__ void k_pass_radius(const float4*, int, const GridHeader*, const int2*, const int*, const VoxelRec*, const float4*,
                              const double*, const AlignState*, AlignState*, double*, unsigned*, double*, PassRecordDev*, int, int,
                              unsigned long long*);
__global__ void k_transform(const float4*, int, const AlignState*, float4*);
__global__ void k_transform_mat(const float4*, int, Mat4f, float4*);
__global__ void k_align_init(const AlignState, AlignState*, unsigned*, unsigned long long*, int, unsigned long long*, const GridHeader*,
                             unsigned long long, const uint4*, uint4*, long long);
__global__ void k_copy16(const uint4*, uint4*, size_t);
__global__ void k_readback(const unsigned long long*, unsigned long long*, int, const unsigned long long*, unsigned long long*, int,
                           const unsigned long long*, unsigned long long*, int, const unsigned long long*, unsigned long long*,
                           unsigned long long*, unsigned long long, unsigned long long*, const GridHeader*);
hipError_t dbg_read_blk(unsigned long long* host, size_t count);
__global__ void k_svd_resume(AlignState*);
template <int SEARCH, bool ONE_TILE>
__global__ void k_pass_lead(const float4*, int, int, const GridHeader*, const int2*, const int*, const VoxelRec*, const AlignState*,
                            AlignState*, const double*, double*, PassRecordDev*, int, unsigned long long*, int4*);
}  // namespace ndt
