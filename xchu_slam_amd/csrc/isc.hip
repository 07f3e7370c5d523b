// isc.hip — Intensity Scan Context kernels (ndt_isc.h): descriptor build, ring masks, loop detection against the device
// database.
#include "ndt_kernels.h"

namespace ndt {

// ground_filter + calculate_isc (ISCGeneration.cpp:284-291, :58-90), the binning pass: every workgroup keeps the cells'
// maxima in LDS (sectors x 64 words, cell = sector * 64 + ring, LDS atomicMax) and merges its non-zero cells into `img`
// (global atomicMax; zeroed before the launch).  A maximum does not depend on the order: deterministic.
__global__ void __launch_bounds__(kIscBlock) k_isc_make(const float4* __restrict__ pts, int n, IscGeom g, unsigned* __restrict__ img) {
    __shared__ unsigned s_cell[kIscMaxSectors * kIscColBytes];
    const int cells = g.sectors * kIscColBytes;
    for (int i = threadIdx.x; i < cells; i += kIscBlock) s_cell[i] = 0u;
    __syncthreads();
    constexpr double kPi = 3.14159265358979323846;
    for (long long i = (long long)blockIdx.x * kIscBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kIscBlock) {
        const float4 p = pts[i];
        // PassThrough on z: non-finite points dropped, both limits inclusive, compared in f32
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
        if (p.z < g.z_min || p.z > g.z_max) continue;
        // sqrtf through f64: the sqrt of an f32 rounded once to f64 and then to f32 is the correctly rounded f32 root
        const double distance = (double)(float)sqrt((double)(p.x * p.x + p.y * p.y));
        if (distance >= g.max_dis) continue;
        const double angle = kPi + (double)(float)atan2((double)p.y, (double)p.x);  // atan2f, modelled
        const double rf = floor(distance / g.ring_step), sf = floor(angle / g.sector_step);
        if (rf >= (double)g.rings || sf >= (double)g.sectors || sf < 0.0) continue;
        const int v = isc_intensity(p.w);
        if (v > 0) atomicMax(&s_cell[(int)sf * kIscColBytes + (int)rf], (unsigned)v);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kIscBlock)
        if (s_cell[i]) atomicMax(&img[i], s_cell[i]);
}

// One workgroup, the new descriptor's: the cell image packs to bytes into slot `slot` (img == nullptr: the slot's columns
// are already in place, ndt_isc_add_descriptor), then one thread per column builds its two ring masks, and the
// keyframe's position and travel distance are stored.
__global__ void __launch_bounds__(kIscBlock) k_isc_finalize(const unsigned* __restrict__ img, IscDb db, int slot, int rings, int sectors,
                                                            double px, double py, double pz, double travel) {
    __shared__ unsigned s_w[kIscMaxSectors * kIscColWords];
    unsigned* cols = reinterpret_cast<unsigned*>(db.cols + (size_t)slot * sectors * kIscColBytes);
    const int words = sectors * kIscColWords;
    for (int w = threadIdx.x; w < words; w += kIscBlock) {
        unsigned v;
        if (img) {
            const uint4 c = reinterpret_cast<const uint4*>(img)[w];
            v = c.x | (c.y << 8) | (c.z << 16) | (c.w << 24);
            cols[w] = v;
        } else {
            v = cols[w];
        }
        s_w[w] = v;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < sectors; c += kIscBlock) {
        unsigned long long zero = 0ull, one = 0ull;
        for (int q = 0; q < rings; ++q) {
            const unsigned b = (s_w[c * kIscColWords + (q >> 2)] >> (8 * (q & 3))) & 255u;
            zero |= (unsigned long long)(b == 0u) << q;
            one |= (unsigned long long)(b == 1u) << q;
        }
        db.zero[(size_t)slot * sectors + c] = zero;
        db.one[(size_t)slot * sectors + c] = one;
    }
    if (threadIdx.x == 0) {
        db.pos[(size_t)slot * 3] = px;
        db.pos[(size_t)slot * 3 + 1] = py;
        db.pos[(size_t)slot * 3 + 2] = pz;
        db.travel[slot] = travel;
    }
}

// detectLoopClosureID (:157-193), one workgroup per (query, chunk of up to 64 candidates): blockIdx.x's query (query[b], or
// q0 when query == nullptr) against the slots blockIdx.y + k * n_chunks that are <= the query — a stride, not a range:
// gated pairs come in runs of neighbouring keyframes (a revisited stretch of road), and a stride deals a run out over
// the workgroups.
// Phase 1, one candidate per thread of wave 0: the f64 gate on travel distance and position.
// Phase 2, one gated pair per wave, its masks and columns staged in the wave's LDS: calculate_geometry_dis (:231-257) — a
// cell pair matches iff both bytes are 0 or both are 1, so a shift's count is the popcount of two mask ANDs per column;
// one shift per lane, the first maximum by a butterfly on (count, lower shift) — and, when the geometry passes,
// calculate_intensity_dis (:259-283): 20 shifts of packed byte SADs over the columns (the padding bytes are 0 on both
// sides), the least.
// Phase 3: the workgroup's best pair under isc_better and its counts, one IscPartial; k_isc_reduce folds the chunks.
// Nothing depends on the order in which pairs are processed.
__global__ void __launch_bounds__(kIscBlock) k_isc_detect(IscDb db, const int* __restrict__ query, int q0, IscDetectArgs a,
                                                          IscPartial* __restrict__ part) {
    __shared__ unsigned long long s_qz[kIscMaxSectors], s_qo[kIscMaxSectors];
    __shared__ unsigned long long s_cz[kIscBlock / 64][kIscMaxSectors], s_co[kIscBlock / 64][kIscMaxSectors];
    __shared__ unsigned s_qc[kIscMaxSectors * kIscColWords], s_cc[kIscBlock / 64][kIscMaxSectors * kIscColWords];
    __shared__ int s_list[kIscChunk];
    __shared__ int s_n;
    __shared__ IscPartial s_best[kIscBlock / 64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int S = a.sectors, R = a.rings;
    const int q = query ? query[blockIdx.x] : q0;
    const bool pair = a.pair_j >= 0;
    IscPartial* out = part + (size_t)blockIdx.x * a.n_chunks + blockIdx.y;
    if (t == 0) s_n = 0;
    __syncthreads();

    // ---- phase 1
    const int i = pair ? a.pair_j : t * a.n_chunks + (int)blockIdx.y;
    bool gated;
    if (pair) {
        gated = t == 0;
    } else {
        gated = false;
        if (t < kIscChunk && i <= q) {
            const double delta = db.travel[q] - db.travel[i];
            const double dx = db.pos[(size_t)i * 3] - db.pos[(size_t)q * 3], dy = db.pos[(size_t)i * 3 + 1] - db.pos[(size_t)q * 3 + 1],
                         dz = db.pos[(size_t)i * 3 + 2] - db.pos[(size_t)q * 3 + 2];
            const double pos = sqrt((dx * dx + dy * dy) + dz * dz);
            gated = delta > a.skip_distance && pos < delta * a.inflation;
        }
    }
    if (gated) s_list[atomicAdd(&s_n, 1)] = i;
    __syncthreads();
    const int ng = s_n;
    if (ng == 0) {
        if (t == 0) *out = IscPartial{0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return;
    }
    const unsigned* qcols = reinterpret_cast<const unsigned*>(db.cols + (size_t)q * S * kIscColBytes);
    for (int w = t; w < S * kIscColWords; w += kIscBlock) s_qc[w] = qcols[w];
    for (int c = t; c < S; c += kIscBlock) {
        s_qz[c] = db.zero[(size_t)q * S + c];
        s_qo[c] = db.one[(size_t)q * S + c];
    }

    // ---- phase 2: the same trip count for every wave (the barriers), a wave past the list idles
    IscPartial best{0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0};
    const double cells = (double)(S * R);
    const int words = S * kIscColWords;
    for (int k0 = 0; k0 < ng; k0 += kIscBlock / 64) {
        const int k = k0 + wave;
        const bool live = k < ng;
        const int c = live ? s_list[k] : 0;
        __syncthreads();  // the previous round's candidates have been read (first round: the query is staged)
        if (live) {
            const unsigned* ccols = reinterpret_cast<const unsigned*>(db.cols + (size_t)c * S * kIscColBytes);
            for (int j = lane; j < words; j += 64) s_cc[wave][j] = ccols[j];
            for (int j = lane; j < S; j += 64) {
                s_cz[wave][j] = db.zero[(size_t)c * S + j];
                s_co[wave][j] = db.one[(size_t)c * S + j];
            }
        }
        __syncthreads();
        if (!live) continue;
        int bcnt = -1, bsh = 0x7fffffff;
        for (int sh = lane; sh < S; sh += 64) {
            int cnt = 0, col = sh;
            for (int p = 0; p < S; ++p) {
                cnt += __popcll(s_qz[p] & s_cz[wave][col]) + __popcll(s_qo[p] & s_co[wave][col]);
                if (++col == S) col = 0;
            }
            if (cnt > bcnt) {  // ascending shifts per lane: the first of equals stays
                bcnt = cnt;
                bsh = sh;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int oc = __shfl_xor(bcnt, o), os = __shfl_xor(bsh, o);
            if (oc > bcnt || (oc == bcnt && os < bsh)) {
                bcnt = oc;
                bsh = os;
            }
        }
        const double geo = (double)bcnt / cells;
        const bool geo_ok = geo > a.geo_thres;
        double inten = 0.0;
        if (geo_ok || pair) {
            const int centre = (pair && a.pair_angle >= 0) ? a.pair_angle : bsh;
            double difference = 1.0;
            for (int d = -kIscWindow; d < kIscWindow; ++d) {
                int shift = (centre + d) % S;
                if (shift < 0) shift += S;
                unsigned sad = 0u;
                for (int item = lane; item < words; item += 64) {  // word `item` of the query against the same word `shift` columns on
                    int other = item + shift * kIscColWords;
                    if (other >= words) other -= words;
                    sad = __builtin_amdgcn_sad_u8(s_qc[item], s_cc[wave][other], sad);
                }
                for (int o = 32; o > 0; o >>= 1) sad += __shfl_xor(sad, o);
                const double diff = (double)sad / (double)(S * R * 255);
                if (diff < difference) difference = diff;
            }
            inten = 1.0 - difference;
        }
        const bool loop = geo_ok && inten > a.inten_thres;
        best.n_geo += geo_ok ? 1 : 0;
        best.n_loop += loop ? 1 : 0;
        if (pair) {
            best.sum = geo + inten;
            best.geo = geo;
            best.inten = inten;
            best.idx = c;
            best.angle = bsh;
        } else if (loop && isc_better(geo + inten, c, best.sum, best.idx)) {
            best.sum = geo + inten;
            best.geo = geo;
            best.inten = inten;
            best.idx = c;
            best.angle = bsh;
        }
    }

    // ---- phase 3
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (t == 0) {
        IscPartial r = s_best[0];
        for (int w = 1; w < kIscBlock / 64; ++w) {
            const IscPartial o = s_best[w];
            r.n_geo += o.n_geo;
            r.n_loop += o.n_loop;
            if (isc_better(o.sum, o.idx, r.sum, r.idx)) {
                r.sum = o.sum;
                r.geo = o.geo;
                r.inten = o.inten;
                r.idx = o.idx;
                r.angle = o.angle;
            }
        }
        r.n_gated = ng;
        *out = r;
    }
}

// The chunks of each query folded in ascending order into its record; "no loop" whenever the winning index is 0.
__global__ void __launch_bounds__(kIscBlock) k_isc_reduce(const IscPartial* __restrict__ part, const int* __restrict__ query, int q0, int n,
                                                          IscDetectArgs a, ndt_isc_result* __restrict__ out) {
    const int b = blockIdx.x * kIscBlock + threadIdx.x;
    if (b >= n) return;
    IscPartial r = part[(size_t)b * a.n_chunks];
    for (int k = 1; k < a.n_chunks; ++k) {
        const IscPartial o = part[(size_t)b * a.n_chunks + k];
        r.n_gated += o.n_gated;
        r.n_geo += o.n_geo;
        r.n_loop += o.n_loop;
        if (isc_better(o.sum, o.idx, r.sum, r.idx)) {
            r.sum = o.sum;
            r.geo = o.geo;
            r.inten = o.inten;
            r.idx = o.idx;
            r.angle = o.angle;
        }
    }
    ndt_isc_result res;
    res.curr_id = query ? query[b] : q0;
    res.best_id = r.idx;
    res.loop_id = (a.pair_j < 0 && r.idx != 0) ? r.idx : -1;
    res.best_score = r.sum;
    res.geo_score = r.geo;
    res.inten_score = r.inten;
    res.angle = r.angle;
    res.n_gated = r.n_gated;
    res.n_geometry = r.n_geo;
    res.n_loop_pairs = r.n_loop;
    out[b] = res;
}

}  // namespace ndt
