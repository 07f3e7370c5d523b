// ground.hip — filter_node's ground detection (xchu_mapping/src/filter_node.cpp:53-216: PlaneClip, NormalFiltering,
// DetectPlane) on the device.  Semantics: DESIGN.md §2 "Ground" (tests/ground_restate.py is their executable form).
//
//   k_ground_clip_flags  the two PlaneClipper3D calls (:113-115) as one flag per point: plane . (x, y, z, 1) >= 0 in f32,
//                        kept by the first plane and not by the second.
//   k_ground_origin      the input index carried beside each float4 through a compaction (k_compact4 moves the points).
//   k_ground_normals<C>  pcl::NormalEstimation (:72-101): one 16-lane team per clipped point over an NNIndex of the
//                        clipped cloud (knn_walk, ndt_nnwalk.h), the k neighbours merged ascending (d2, index), f64 mean
//                        and moments in that order, sym_eigen3, the flip to the viewpoint and the keep flag in one launch.
//   k_ground_sample      SampleConsensusModel::getSamples for one batch of hypotheses: one lane replays drawIndexSample's
//                        partial Fisher-Yates over shuffled_indices_ (three entries in registers, every other touched
//                        entry in a hash) from the uploaded generator table, and redraws while isSampleGood fails.
//   k_ground_score       one batch: every workgroup derives the batch's plane coefficients (computeModelCoefficients),
//                        each point is read once and tested against all of them, counts through wave shuffles and
//                        last_workgroup_sums; the last workgroup replays RandomSampleConsensus::computeModel's
//                        sequential rule over the batch.  A launch after the loop has ended returns at its first load.
//   k_ground_finish      selectWithinDistance of the winner, the gates of :158-177, the result record, the ground flags
//                        and the marks of the input points the ground came from.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "ndt_device.h"
#include "ndt_ground.h"
#include "ndt_nnwalk.h"
#include "ndt_lastwg.h"
#include "ndt_kernels.h"
#include "../../include/ndt_hip.h"

namespace ndt {

namespace {

static_assert(kGroundTeam == kNnTeam, "k_ground_normals' teams are knn_walk's");
static_assert(kGroundBatch <= 64 && kGroundBatch <= kGroundBlock, "one thread per hypothesis; last_workgroup_sums takes 64 sums");

// SampleConsensusModelPlane: the f32 distance of a point to a plane, ((a x + b y) + c z) + d
__device__ __forceinline__ float plane_dist(const float4 m, const float4 p) { return ((m.x * p.x + m.y * p.y) + m.z * p.z) + m.w; }

// fabs(distance) < threshold: the float's magnitude against the double threshold, as countWithinDistance compares
__device__ __forceinline__ bool plane_inlier(const float4 m, const float4 p, double thr) { return (double)fabsf(plane_dist(m, p)) < thr; }

// isSampleGood / computeModelCoefficients: the component-wise ratios of p1 - p0 and p2 - p0 all equal (a NaN ratio is
// unequal to everything: such a sample passes, as it does in the reference)
__device__ __forceinline__ bool collinear(const float4 p0, const float4 p1, const float4 p2) {
    const float r0 = (p1.x - p0.x) / (p2.x - p0.x), r1 = (p1.y - p0.y) / (p2.y - p0.y), r2 = (p1.z - p0.z) / (p2.z - p0.z);
    return r0 == r1 && r2 == r1;
}

// computeModelCoefficients: the f32 cross product of the two differences, normalised, d = -(n . p0)
__device__ __forceinline__ float4 plane_of(const float4 p0, const float4 p1, const float4 p2) {
    const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
    const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
    float4 m;
    m.x = ay * bz - az * by;
    m.y = az * bx - ax * bz;
    m.z = ax * by - ay * bx;
    const float nrm = sqrtf((m.x * m.x + m.y * m.y) + m.z * m.z);
    m.x /= nrm;
    m.y /= nrm;
    m.z /= nrm;
    m.w = -((m.x * p0.x + m.y * p0.y) + m.z * p0.z);
    return m;
}

__device__ __forceinline__ unsigned ground_slot(int j, int mask) { return ((unsigned)j * 2654435761u >> 7) & (unsigned)mask; }

// shuffled_indices_[j] for j >= 3: the hash's entry, or j itself while the position is untouched
__device__ __forceinline__ int shuffled_get(const int2* __restrict__ hash, int mask, int j) {
    unsigned s = ground_slot(j, mask);
    for (int probe = 0; probe <= mask; ++probe, s = (s + 1) & (unsigned)mask) {
        const int2 e = hash[s];
        if (e.x == j) return e.y;
        if (e.x < 0) break;
    }
    return j;
}

__device__ __forceinline__ void shuffled_set(int2* __restrict__ hash, int mask, int j, int v) {
    unsigned s = ground_slot(j, mask);
    for (int probe = 0; probe <= mask; ++probe, s = (s + 1) & (unsigned)mask) {
        const int k = hash[s].x;
        if (k == j || k < 0) {
            hash[s] = make_int2(j, v);
            return;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kGroundBlock) void k_ground_clip_flags(const float4* __restrict__ in, int n, float d_keep, float d_drop,
                                                                    int* __restrict__ flags) {
    for (int i = blockIdx.x * kGroundBlock + threadIdx.x; i < n; i += gridDim.x * kGroundBlock) {
        const float4 p = in[i];
        // PlaneClipper3D with the planes (0, 0, 1, d): the dot product as written, the zero products included
        const float a = ((0.f * p.x + 0.f * p.y) + 1.f * p.z) + d_keep;
        const float b = ((0.f * p.x + 0.f * p.y) + 1.f * p.z) + d_drop;
        flags[i] = (a >= 0.f && !(b >= 0.f)) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_origin(const int* __restrict__ flags, const int* __restrict__ idx,
                                                                const int* __restrict__ org_in, int n, int* __restrict__ org_out) {
    for (int i = blockIdx.x * kGroundBlock + threadIdx.x; i < n; i += gridDim.x * kGroundBlock)
        if (flags[i]) org_out[idx[i]] = org_in ? org_in[i] : i;
}

template <int C>
__global__ __launch_bounds__(kGroundBlock) void k_ground_normals(const float4* __restrict__ pts, int n, int k, int k_stride, float vp_z,
                                                                 double cos_thr, const GridHeader* __restrict__ h,
                                                                 const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                                                 const float4* __restrict__ ix_pts, const int* __restrict__ ix_idx,
                                                                 float4* __restrict__ normal4, int* __restrict__ flags,
                                                                 int* __restrict__ nbr) {
    if (!h) {  // use_normal_filtering = false: every clipped point stays
        for (int i = blockIdx.x * kGroundBlock + threadIdx.x; i < n; i += gridDim.x * kGroundBlock) {
            flags[i] = 1;
            normal4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const int db[3] = {h->div_b[0], h->div_b[1], h->div_b[2]};
    const int nbk[3] = {h->nblk[0], h->nblk[1], h->nblk[2]};
    const float cell = h->leaf[0];
    const int t = threadIdx.x % kGroundTeam;
    for (int i = blockIdx.x * kGroundTeams + threadIdx.x / kGroundTeam; i < n; i += gridDim.x * kGroundTeams) {
        const float4 p = pts[i];
        const float q[3] = {p.x, p.y, p.z};
        KnnList<C> top;
        knn_walk<C>(q, t, k, h, db, nbk, cell, block_table, cell_off, ix_pts, ix_idx, top);
        // the k neighbours ascending (d2, index); the sums run in that order, every lane keeping all of them
        double mean[3] = {0.0, 0.0, 0.0};
        double c00 = 0.0, c10 = 0.0, c11 = 0.0, c20 = 0.0, c21 = 0.0, c22 = 0.0;
        int cnt = 0;
        for (int r = 0; r < k; ++r) {
            const unsigned long long m = knn_next<C>(top);
            if (m == kKnnNone) break;
            const int j = (int)(unsigned)(m & 0xffffffffull);
            if (t == 0) nbr[(size_t)i * k_stride + r] = j;
            const float4 pt = pts[j];
            mean[0] += (double)pt.x;
            mean[1] += (double)pt.y;
            mean[2] += (double)pt.z;
            c00 += (double)(pt.x * pt.x);  // f32 products added to f64 sums, as k_gicp_cov
            c10 += (double)(pt.y * pt.x);
            c11 += (double)(pt.y * pt.y);
            c20 += (double)(pt.z * pt.x);
            c21 += (double)(pt.z * pt.y);
            c22 += (double)(pt.z * pt.z);
            ++cnt;
        }
        if (t == 0) {
            for (int r = cnt; r < k_stride; ++r) nbr[(size_t)i * k_stride + r] = -1;
            float nx = NAN, ny = NAN, nz = NAN, az = NAN;
            int keep = 0;
            if (cnt >= 3) {  // computePointNormal: fewer than three neighbours leave the normal NaN
                const double kd = (double)cnt;
                for (int a = 0; a < 3; ++a) mean[a] /= kd;
                double A[9];  // column-major; sym_eigen3 reads the lower triangle
                A[0] = c00 / kd - mean[0] * mean[0];
                A[1] = c10 / kd - mean[1] * mean[0];
                A[2] = c20 / kd - mean[2] * mean[0];
                A[4] = c11 / kd - mean[1] * mean[1];
                A[5] = c21 / kd - mean[2] * mean[1];
                A[8] = c22 / kd - mean[2] * mean[2];
                A[3] = A[1]; A[6] = A[2]; A[7] = A[5];
                double ev[3], Q[9];
                (void)sym_eigen3(A, ev, Q);
                nx = (float)Q[0]; ny = (float)Q[1]; nz = (float)Q[2];  // the smallest eigenvalue's vector
                // flipNormalTowardsViewpoint, viewpoint (0, 0, sensor_height)
                const float vx = 0.f - p.x, vy = 0.f - p.y, vz = vp_z - p.z;
                if ((vx * nx + vy * ny) + vz * nz < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
                // getNormalVector3fMap().normalized().dot(UnitZ) in f32, compared in double
                const float nrm = sqrtf((nx * nx + ny * ny) + nz * nz);
                const float dot = ((nx / nrm) * 0.f + (ny / nrm) * 0.f) + (nz / nrm) * 1.f;
                az = fabsf(dot);
                keep = (double)az > cos_thr ? 1 : 0;
            }
            normal4[i] = make_float4(nx, ny, nz, az);
            flags[i] = keep;
        }
    }
}

template __global__ void k_ground_normals<10>(const float4*, int, int, int, float, double, const GridHeader*, const int*, const int*,
                                              const float4*, const int*, float4*, int*, int*);
template __global__ void k_ground_normals<20>(const float4*, int, int, int, float, double, const GridHeader*, const int*, const int*,
                                              const float4*, const int*, float4*, int*, int*);

__global__ __launch_bounds__(64) void k_ground_sample(const float4* __restrict__ pts, GroundState* __restrict__ st, int batch,
                                                      const unsigned* __restrict__ table, int2* __restrict__ hash,
                                                      int4* __restrict__ tri) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st->done) return;
    const int n = st->n_normal;
    if (n < st->floor_pts || n < 3) {  // "too few points for RANSAC" (:144): the gate is taken here, no count goes to the host
        st->done = 1;
        return;
    }
    if (st->inject) return;  // the caller's samples (ndt_ground_set_samples) are in tri already
    const int words = st->stream_words, mask = st->hash_mask;
    int s[3] = {st->s[0], st->s[1], st->s[2]};
    int pos = st->stream_pos;
    for (int hyp = 0; hyp < kGroundBatch; ++hyp) {
        bool good = false, over = false;
        for (int check = 0; check < kGroundSampleChecks && !good; ++check) {
            if (pos + 3 > words) {
                over = true;
                break;
            }
            // rnd(): boost::uniform_int<>(0, INT_MAX) over mt19937, modelled as the raw word shifted right by one
            const unsigned r[3] = {table[pos] >> 1, table[pos + 1] >> 1, table[pos + 2] >> 1};
            pos += 3;
            // drawIndexSample: swap(shuffled[i], shuffled[i + rnd() % (n - i)]) for i = 0, 1, 2
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int j = i + (int)(r[i] % (unsigned)(n - i));
                if (j == i) continue;
                if (j < 3) {  // i < j <= 2
                    const int sj = j == 1 ? s[1] : s[2];
                    if (j == 1) s[1] = s[i]; else s[2] = s[i];
                    s[i] = sj;
                } else {
                    const int v = shuffled_get(hash, mask, j);
                    shuffled_set(hash, mask, j, s[i]);
                    s[i] = v;
                }
            }
            good = !collinear(pts[s[0]], pts[s[1]], pts[s[2]]);
        }
        if (over) {  // the table ended: the host continues the stream and runs the scan's loop again
            st->overrun = 1;
            st->done = 1;
            break;
        }
        if (!good) break;  // "No samples could be selected": the entry stays GROUND_SAMPLE_NONE and ends the loop
        tri[batch * kGroundBatch + hyp] = make_int4(s[0], s[1], s[2], GROUND_SAMPLE_OK);
        st->made = batch * kGroundBatch + hyp + 1;
    }
    st->s[0] = s[0]; st->s[1] = s[1]; st->s[2] = s[2];
    st->stream_pos = pos;
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_score(const float4* __restrict__ pts, GroundState* __restrict__ st, int batch,
                                                               const int4* __restrict__ tri, float4* __restrict__ coef,
                                                               int* __restrict__ stat, int* __restrict__ cnt_out,
                                                               double* __restrict__ partials, unsigned* __restrict__ ticket) {
    // the state is rewritten by this launch's last workgroup only after every workgroup has taken its ticket
    if (st->done) return;
    const int n = st->n_normal;
    const double thr = st->thr;
    __shared__ float4 s_coef[kGroundBatch];
    __shared__ int s_stat[kGroundBatch];
    if (threadIdx.x < kGroundBatch) {
        const int4 tr = tri[batch * kGroundBatch + threadIdx.x];
        int status = GROUND_SAMPLE_NONE;
        float4 m = make_float4(NAN, NAN, NAN, NAN);  // a NaN plane has no inliers
        if (tr.x >= 0 && tr.y >= 0 && tr.z >= 0 && tr.x < n && tr.y < n && tr.z < n) {
            const float4 p0 = pts[tr.x], p1 = pts[tr.y], p2 = pts[tr.z];
            status = collinear(p0, p1, p2) ? GROUND_SAMPLE_DEGENERATE : GROUND_SAMPLE_OK;
            if (status == GROUND_SAMPLE_OK) m = plane_of(p0, p1, p2);
        }
        s_coef[threadIdx.x] = m;
        s_stat[threadIdx.x] = status;
        if (blockIdx.x == 0) {
            coef[batch * kGroundBatch + threadIdx.x] = m;
            stat[batch * kGroundBatch + threadIdx.x] = status;
        }
    }
    __syncthreads();
    int c[kGroundBatch];
#pragma unroll
    for (int hyp = 0; hyp < kGroundBatch; ++hyp) c[hyp] = 0;
    for (int i = blockIdx.x * kGroundBlock + threadIdx.x; i < n; i += gridDim.x * kGroundBlock) {
        const float4 p = pts[i];
#pragma unroll
        for (int hyp = 0; hyp < kGroundBatch; ++hyp) c[hyp] += plane_inlier(s_coef[hyp], p, thr) ? 1 : 0;
    }
    constexpr int kWaves = kGroundBlock / 64;
    __shared__ double s_part[kWaves][kGroundBatch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int hyp = 0; hyp < kGroundBatch; ++hyp) {
        int v = c[hyp];
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_part[wave][hyp] = (double)v;  // counts below 2^31 are exact in f64, and so are their sums
    }
    double S[kGroundBatch];
    __shared__ double s_total[kGroundBatch];  // the replay below indexes the totals by a loop variable: LDS, not registers
    if (!last_workgroup_sums<kGroundBatch, kGroundBlock>(s_part, partials, ticket, S)) return;
#pragma unroll
    for (int hyp = 0; hyp < kGroundBatch; ++hyp) s_total[hyp] = S[hyp];
    // ---- RandomSampleConsensus::computeModel's loop over this batch's hypotheses, in order
    int best_cnt = st->best_cnt, best_h = st->best_h, iterations = st->iterations, skipped = st->skipped, seen = st->seen;
    double k = st->k;
    const double one_over_n = 1.0 / (double)n;
    int done = 0;
    for (int hyp = 0; hyp < kGroundBatch && !done; ++hyp) {
        const int gi = batch * kGroundBatch + hyp;
        const int status = s_stat[hyp];
        cnt_out[gi] = (int)s_total[hyp];
        if (status == GROUND_SAMPLE_NONE) {  // no sample: the loop breaks
            done = 1;
            break;
        }
        ++seen;
        if (status == GROUND_SAMPLE_DEGENERATE) {  // computeModelCoefficients failed: skipped, not an iteration
            if (++skipped >= st->max_skip) done = 1;
            continue;
        }
        const int count = (int)s_total[hyp];
        if (count > best_cnt) {
            best_cnt = count;
            best_h = gi;
            const double w = (double)count * one_over_n;
            double p_no_outliers = 1.0 - (w * w) * w;
            p_no_outliers = fmax(DBL_EPSILON, p_no_outliers);
            p_no_outliers = fmin(1.0 - DBL_EPSILON, p_no_outliers);
            k = st->log_prob / log(p_no_outliers);
        }
        ++iterations;
        if (iterations > st->max_it) done = 1;     // "reached the maximum number of trials"
        if (!((double)iterations < k)) done = 1;   // while (iterations_ < k)
    }
    st->best_cnt = best_cnt;
    st->best_h = best_h;
    st->iterations = iterations;
    st->skipped = skipped;
    st->seen = seen;
    st->k = k;
    st->done = done;
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_finish(const float4* __restrict__ pts, const int* __restrict__ org, int cap,
                                                                GroundState* __restrict__ st, const int4* __restrict__ tri,
                                                                const float4* __restrict__ coef, int* __restrict__ gflag,
                                                                int* __restrict__ mark) {
    if (!st->done || st->overrun) return;
    const int n = min(st->n_normal, cap);
    const int floor_pts = st->floor_pts, best_h = st->best_h, best_cnt = st->best_cnt;
    int reason = NDT_GROUND_OK;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < floor_pts || n < 3) reason = NDT_GROUND_TOO_FEW_POINTS;
    else if (best_h < 0 || best_cnt < floor_pts) reason = NDT_GROUND_TOO_FEW_INLIERS;
    if (best_h >= 0) m = coef[best_h];
    if (reason == NDT_GROUND_OK) {
        // |coeffs.head3 . (T^-1 UnitZ).head3| against cos(floor_normal_thresh): the f32 dot product, compared in double
        const float dot = (m.x * st->ref[0] + m.y * st->ref[1]) + m.z * st->ref[2];
        if (fabs((double)dot) < st->cos_floor) reason = NDT_GROUND_NOT_VERTICAL;
    }
    const bool found = reason == NDT_GROUND_OK;
    const bool literal = st->literal != 0;
    const int n_input = st->n_input;
    const double thr = st->thr;
    for (int j = blockIdx.x * kGroundBlock + threadIdx.x; j < n; j += gridDim.x * kGroundBlock) {
        const bool in = found && plane_inlier(m, pts[j], thr);  // selectWithinDistance, in index order
        gflag[j] = in ? 1 : 0;
        if (in) {
            // /no_ground_points: the input point this inlier came from, or (the reference's form) the input point that
            // has the inlier's index in the filtered cloud
            const int at = literal ? j : org[j];
            if (at >= 0 && at < n_input) mark[at] = 1;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->found = found ? 1 : 0;
        st->reason = reason;
        st->n_inliers = best_h >= 0 ? best_cnt : 0;
        // make the normal upward: coeffs.head3 . UnitZ < 0 negates all four
        const bool neg = found && (m.x * 0.f + m.y * 0.f) + m.z * 1.f < 0.f;
        st->coeffs[0] = found ? (neg ? -m.x : m.x) : 0.f;
        st->coeffs[1] = found ? (neg ? -m.y : m.y) : 0.f;
        st->coeffs[2] = found ? (neg ? -m.z : m.z) : 0.f;
        st->coeffs[3] = found ? (neg ? -m.w : m.w) : 0.f;
        const int4 tr = best_h >= 0 ? tri[best_h] : make_int4(-1, -1, -1, -1);
        st->winner[0] = best_h >= 0 && tr.x >= 0 && tr.x < n ? org[tr.x] : -1;
        st->winner[1] = best_h >= 0 && tr.y >= 0 && tr.y < n ? org[tr.y] : -1;
        st->winner[2] = best_h >= 0 && tr.z >= 0 && tr.z < n ? org[tr.z] : -1;
    }
}

// the flags of /no_ground_points over the input cloud: every point k_ground_finish did not mark
__global__ __launch_bounds__(kGroundBlock) void k_ground_unmarked(const int* __restrict__ mark, int n, int* __restrict__ flags) {
    for (int i = blockIdx.x * kGroundBlock + threadIdx.x; i < n; i += gridDim.x * kGroundBlock) flags[i] = mark[i] ? 0 : 1;
}

}  // namespace ndt
