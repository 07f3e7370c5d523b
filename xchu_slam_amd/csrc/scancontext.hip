// scancontext.hip — Scan Context kernels (ndt_sc.h): descriptor build, keys, loop detection against the device database.
#include "ndt_kernels.h"

namespace ndt {

// makeScancontext (Scancontext.cpp:151-195), the binning pass: every workgroup keeps the 1200 bins in LDS as
// order-preserving images of z + lidar height (4.8 KB, LDS atomicMax) and merges its non-empty bins into `bins` (global
// atomicMax; set to the image of NO_POINT before the launch).  A maximum does not depend on the order: deterministic.
__global__ void __launch_bounds__(kScBlock) k_sc_make(const float4* __restrict__ pts, int n, unsigned* __restrict__ bins) {
    __shared__ unsigned s_bin[kScBins];
    const unsigned empty = sc_image(kScNoPoint);
    for (int i = threadIdx.x; i < kScBins; i += kScBlock) s_bin[i] = empty;
    __syncthreads();
    constexpr double kDeg = 180 / 3.14159265358979323846;  // (180/M_PI)
    for (long long i = (long long)blockIdx.x * kScBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kScBlock) {
        const float4 p = pts[i];
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;  // outside the contract: skipped
        const float zp = (float)((double)p.z + kScLidarHeight);
        // sqrtf and the f32 quotient through f64: sqrt and / of f32 values rounded once to f64 and then to f32 are the
        // correctly rounded f32 results (53 >= 2 * 24 + 2)
        const float r = (float)sqrt((double)(p.x * p.x + p.y * p.y));
        if (r > (float)kScMaxRadius) continue;
        // xy2theta (:23-36): atanf of an f32 quotient, scaled and placed per quadrant in f64, narrowed on return
        const bool xn = p.x < 0.f, yn = p.y < 0.f;
        const float num = (!xn && yn) ? -p.y : p.y;
        const float den = (xn && !yn) ? -p.x : p.x;
        const float q = (float)((double)num / (double)den);
        const double ka = kDeg * (double)(float)atan((double)q);
        const float theta = (float)(!xn ? (!yn ? ka : 360.0 - ka) : (!yn ? 180.0 - ka : 180.0 + ka));
        const int ring = sc_ceil_clamp(((double)r / kScMaxRadius) * kScRings, kScRings);
        const int sector = sc_ceil_clamp(((double)theta / 360.0) * kScSectors, kScSectors);
        atomicMax(&s_bin[(sector - 1) * kScRings + (ring - 1)], sc_image(zp));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kScBins; i += kScBlock)
        if (s_bin[i] > empty) atomicMax(&bins[i], s_bin[i]);
}

// One workgroup, the new descriptor's: NO_POINT bins become 0 and widen to double into slot `slot` (bins == nullptr:
// the slot's descriptor is already in place, saveScancontextAndKeys), then the ring key (row means, f32), the sector key
// (column means) and the column norms, each reduction in the order of sc_esum.
__global__ void __launch_bounds__(kScBlock) k_sc_finalize(const unsigned* __restrict__ bins, ScDb db, int slot) {
    __shared__ double s_d[kScBins];
    double* desc = db.desc + (size_t)slot * kScBins;
    for (int i = threadIdx.x; i < kScBins; i += kScBlock) {
        double v;
        if (bins) {
            const float f = sc_unimage(bins[i]);
            v = f == kScNoPoint ? 0.0 : (double)f;
            desc[i] = v;
        } else {
            v = desc[i];
        }
        s_d[i] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kScRings) {
        const double sum = sc_esum(kScSectors, [&](int j) { return s_d[j * kScRings + t]; });
        db.ringkey[(size_t)slot * kScRings + t] = (float)(sum / (double)kScSectors);
    } else if (t >= 64 && t < 64 + kScSectors) {
        const int c = t - 64;
        const double sum = sc_esum(kScRings, [&](int r) { return s_d[c * kScRings + r]; });
        db.sectorkey[(size_t)slot * kScSectors + c] = sum / (double)kScRings;
    } else if (t >= 128 && t < 128 + kScSectors) {
        const int c = t - 128;
        const double sq = sc_esum(kScRings, [&](int r) { return s_d[c * kScRings + r] * s_d[c * kScRings + r]; });
        db.colnorm[(size_t)slot * kScSectors + c] = sqrt(sq);
    }
}

// a shift of the search space: within `radius` of the sector-key argmin `a`, around the circle
__device__ inline bool sc_in_space(int s, int a, int radius) {
    const int d = (s - a + kScSectors) % kScSectors;
    return d <= radius || kScSectors - d <= radius;
}

// The reference's "first minimum below 10000000" scan (strict <, so a NaN never wins) over the wave's candidate lanes, as
// one butterfly: the least (value, index) pair, in every lane; (10000000, 0) when no lane qualifies.
__device__ inline void sc_first_min(double v, int idx, bool cand, double* best, int* arg) {
    const bool ok = cand && v < kScBig;
    double bv = ok ? v : HUGE_VAL;
    int bi = ok ? idx : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov < bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    *best = bi == 0x7fffffff ? kScBig : bv;
    *arg = bi == 0x7fffffff ? 0 : bi;
}

// detectLoopClosureID (:331-422) after its early return, one workgroup per query (blockIdx.x): query[b] (or q0 when
// query == nullptr) against the ring keys [0, n_search[b]) (or ns0).  Phase 1: the num_candidates nearest ring keys under
// nanoflann's f32 L2_Adaptor by repeated argmin (equal distances to the lower index; the distances are recomputed per
// round, 20 f32 per key).  Phase 2, per candidate in ascending distance: distanceBtnScanContext (:116-148) — the 60-shift
// sector-key alignment (one shift per lane of wave 0, first minimum by sc_first_min), then distDirectSC for the shifts of
// the search space, one wave per shift: the per-column dots in parallel, lane = column, and the similarity sum in column
// order over lane broadcasts (no LDS, no barrier).  One ndt_sc_result per query.
__global__ void __launch_bounds__(kScBlock) k_sc_detect(ScDb db, const int* __restrict__ query, const int* __restrict__ n_search, int q0,
                                                        int ns0, ScDetectArgs a, ndt_sc_result* __restrict__ out) {
    __shared__ double s_q[kScBins], s_c[kScBins];
    __shared__ double s_qn[kScSectors], s_cn[kScSectors], s_qk[kScSectors], s_ck[kScSectors];
    __shared__ double s_sd[kScSectors];
    __shared__ float s_rk[kScRings];
    __shared__ float s_rd[kScBlock / 64];
    __shared__ int s_ri[kScBlock / 64];
    __shared__ int s_cand[kScMaxCand];
    __shared__ int s_ncand, s_arg;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int q = query ? query[blockIdx.x] : q0;
    const int ns = n_search ? n_search[blockIdx.x] : ns0;
    ndt_sc_result* res = out + blockIdx.x;
    if (t == 0) {
        res->loop_id = -1;
        res->yaw_diff = 0.f;
        res->min_dist = kScBig;
        res->nn_idx = 0;
        res->nn_align = 0;
        res->n_candidates = 0;
        for (int k = 0; k < kScMaxCand; ++k) {
            res->cand_idx[k] = -1;
            res->cand_dist[k] = 0.0;
            res->cand_shift[k] = 0;
        }
    }
    if (a.pair_j < 0 && ns <= 0) return;  // fewer than num_exclude_recent + 1 descriptors: (-1, 0.0f)

    for (int i = t; i < kScBins; i += kScBlock) s_q[i] = db.desc[(size_t)q * kScBins + i];
    if (t < kScSectors) {
        s_qn[t] = db.colnorm[(size_t)q * kScSectors + t];
        s_qk[t] = db.sectorkey[(size_t)q * kScSectors + t];
    }
    if (t < kScRings) s_rk[t] = db.ringkey[(size_t)q * kScRings + t];
    __syncthreads();

    // ---- phase 1
    if (a.pair_j >= 0) {
        if (t == 0) {
            s_cand[0] = a.pair_j;
            s_ncand = 1;
        }
    } else {
        float pd = -1.f;  // the previous round's pick: this round takes the least (distance, index) after it
        int pi = -1;
        if (t == 0) s_ncand = 0;
        for (int k = 0; k < a.num_candidates; ++k) {
            float bd = 0.f;
            int bi = -1;
            for (int i = t; i < ns; i += kScBlock) {
                const float* kp = db.ringkey + (size_t)i * kScRings;
                float d2 = 0.f;
                for (int g = 0; g < kScRings; g += 4) {
                    const float d0 = s_rk[g] - kp[g], d1 = s_rk[g + 1] - kp[g + 1], d2_ = s_rk[g + 2] - kp[g + 2], d3 = s_rk[g + 3] - kp[g + 3];
                    d2 += d0 * d0 + d1 * d1 + d2_ * d2_ + d3 * d3;
                }
                const bool after = d2 > pd || (d2 == pd && i > pi);
                if (after && (bi < 0 || d2 < bd)) {  // ascending i per thread: the first of equals stays
                    bd = d2;
                    bi = i;
                }
            }
            // the least (distance, index) pair of the workgroup: a butterfly per wave, then the four waves' pairs
            for (int o = 32; o > 0; o >>= 1) {
                const float od = __shfl_xor(bd, o);
                const int oi = __shfl_xor(bi, o);
                if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) {
                    bd = od;
                    bi = oi;
                }
            }
            if (lane == 0) {
                s_rd[wave] = bd;
                s_ri[wave] = bi;
            }
            __syncthreads();
            pd = 0.f;
            pi = -1;
            for (int w = 0; w < kScBlock / 64; ++w) {
                const float od = s_rd[w];
                const int oi = s_ri[w];
                if (oi >= 0 && (pi < 0 || od < pd || (od == pd && oi < pi))) {
                    pd = od;
                    pi = oi;
                }
            }
            __syncthreads();
            if (pi < 0) break;  // fewer keys than candidates: the keys found
            if (t == 0) {
                s_cand[k] = pi;
                s_ncand = k + 1;
            }
        }
    }
    __syncthreads();
    const int ncand = s_ncand;

    // ---- phase 2
    double min_dist = kScBig;
    int nn_align = 0, nn_idx = 0;
    for (int k = 0; k < ncand; ++k) {
        const int c = s_cand[k];
        for (int i = t; i < kScBins; i += kScBlock) s_c[i] = db.desc[(size_t)c * kScBins + i];
        if (t < kScSectors) {
            s_cn[t] = db.colnorm[(size_t)c * kScSectors + t];
            s_ck[t] = db.sectorkey[(size_t)c * kScSectors + t];
        }
        __syncthreads();
        // fastAlignUsingVkey (:93-113): |vkey1 - circshift(vkey2, s)| for the 60 shifts, first minimum
        if (wave == 0) {
            const int sh = lane < kScSectors ? lane : 0;
            const double sq = sc_esum(kScSectors, [&](int j) {
                const double d = s_qk[j] - s_ck[(j - sh + kScSectors) % kScSectors];
                return d * d;
            });
            double best;
            int arg;
            sc_first_min(sqrt(sq), lane, lane < kScSectors, &best, &arg);
            if (lane == 0) s_arg = arg;
        }
        __syncthreads();
        const int arg0 = s_arg;
        // distDirectSC (:69-90) of the shifts in the search space, in ascending order: the m-th goes to wave m % 4
        int m = 0;
        for (int s = 0; s < kScSectors; ++s) {
            if (!sc_in_space(s, arg0, a.radius)) continue;  // the same for every thread
            if ((m++ & (kScBlock / 64 - 1)) != wave) continue;
            const bool col = lane < kScSectors;
            const int cj = (lane - s + 2 * kScSectors) % kScSectors;  // circshift: column `lane` of the shifted = column cj
            const double n1 = col ? s_qn[lane] : 0.0, n2 = s_cn[cj];
            const bool valid = col && !(n1 == 0.0 || n2 == 0.0);
            double sim = 0.0;
            if (valid) {
                const double dot = sc_esum(kScRings, [&](int r) { return s_q[lane * kScRings + r] * s_c[cj * kScRings + r]; });
                sim = dot / (n1 * n2);
            }
            const unsigned long long counted = __ballot(valid);
            double total = 0.0;  // every lane adds the columns' similarities in column order
            for (int j = 0; j < kScSectors; ++j) {
                const double v = __shfl(sim, j);
                if ((counted >> j) & 1ull) total = total + v;
            }
            if (lane == 0) s_sd[s] = 1.0 - total / (double)__popcll(counted);  // no column counted: NaN, which never wins a <
        }
        __syncthreads();
        if (wave == 0) {
            double best;
            int arg;
            const bool in = lane < kScSectors && sc_in_space(lane, arg0, a.radius);
            sc_first_min(in ? s_sd[lane] : 0.0, lane, in, &best, &arg);
            if (lane == 0) {
                res->cand_idx[k] = c;
                res->cand_dist[k] = best;
                res->cand_shift[k] = arg;
                if (best < min_dist) {
                    min_dist = best;
                    nn_align = arg;
                    nn_idx = c;
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        res->n_candidates = ncand;
        res->min_dist = min_dist;
        res->nn_idx = nn_idx;
        res->nn_align = nn_align;
        res->loop_id = min_dist < a.dist_thres ? nn_idx : -1;
        // deg2rad (:17-20) of nn_align * PC_UNIT_SECTORANGLE, both narrowed through float
        const float deg = (float)((double)nn_align * (360.0 / (double)kScSectors));
        res->yaw_diff = (float)((double)deg * 3.14159265358979323846 / 180.0);
    }
}

}  // namespace ndt
