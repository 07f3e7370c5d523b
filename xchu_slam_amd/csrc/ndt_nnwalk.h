// ndt_nnwalk.h — the exact nearest-neighbour walk of one 16-lane team over an NNIndex (device only): the 3x3x3 cube
// around the query cell, the 5x5x5 cube, then shells of 8x8x8-cell blocks.  The one copy of that walk, shared by
// k_fitness (fitness.hip), k_icp_pass (icp.hip) and k_gicp_pairs (gicp.hip).
//
// What a caller keeps of the candidates is its tracker's business.  A tracker supplies take(d, j, ix) (candidate j of
// the index at squared distance d), team(ix) (the 16-lane reduce that leaves it team-uniform), the current distance d,
// the two comparisons the walk stops and prunes by, settled(bound2) and skip(lb), and index(): the index's fifth word
// if it reads one.  The walk takes that pointer from the tracker once and hands it back as ix: read through the
// tracker's reference at every candidate instead, the compiler allocates k_icp_pass's registers differently (same
// count) and the pass comes out 0.8 % slower; this way its code is the walk's code of before the trackers.
//   NnMin  (getFitnessScore) keeps the minimum alone.  A point that could only tie changes nothing, so the walk may
//          stop at best <= bound^2 and pass over a block whose lower bound equals the best.
//   NnArg  (ICP, GICP) keeps the argmin; equal f32 distances go to the lowest index in the caller's order (the index
//          build carries that index as a fifth word beside the sorted points).  A point that could only tie may still
//          win on its index and must be seen: the walk stops only at best < bound^2 and passes over a block only when
//          its lower bound is above the best.
// Distances are FLANN's L2_Simple in f32, (dx^2 + dy^2) + dz^2; the minimum depends neither on the visiting order nor on
// the lane split, and with the tie rule neither does the argmin.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "ndt_types.h"

namespace ndt {

constexpr int kNnTeam = kFitTeam;  // lanes per query (ndt_types.h)
constexpr int kNnU = 8;                // point loads in flight per lane (clamped repeats past a range's end)
constexpr int kNnCells = 2;            // ring-cube cells per lane per step: their table, offset and point loads issued together

// FLANN L2_Simple in f32
__device__ __forceinline__ float nn_l2(const float4 t, const float q[3]) {
    float d = 0.f, u;
    u = t.x - q[0]; d += u * u;
    u = t.y - q[1]; d += u * u;
    u = t.z - q[2]; d += u * u;
    return d;
}

// running minimum of one lane
struct NnMin {
    float d;
    __device__ __forceinline__ const int* index() const { return nullptr; }  // reads no fifth word
    // a repeated candidate is harmless for a minimum
    __device__ __forceinline__ void take(float v, int, const int*) { d = fminf(d, v); }
    __device__ __forceinline__ void team(const int*) {
        for (int m = kNnTeam / 2; m > 0; m >>= 1) d = fminf(d, __shfl_xor(d, m, kNnTeam));
    }
    // every unvisited point is at least sqrt(bound2) away: none can be closer, and one as close leaves the minimum as it is
    __device__ __forceinline__ bool settled(float bound2) const { return d <= bound2; }
    // a block no closer than the minimum cannot lower it
    __device__ __forceinline__ bool skip(float lb) const { return lb >= d; }
};

// running argmin of one lane: squared distance, position in the index, original target index (-2: not loaded yet),
// and the index's fifth word (per sorted point: its index in the caller's order).  Starts as {INFINITY, -1, INT_MAX, idx};
// pos stays -1 when no point was found.
struct NnArg {
    float d;
    int pos, orig;
    const int* __restrict__ idx;
    __device__ __forceinline__ const int* index() const { return idx; }
    // candidate j at distance v; a tie goes to the lower original index (loaded only then); a repeated j changes nothing
    __device__ __forceinline__ void take(float v, int j, const int* __restrict__ ix) {
        if (v < d) {
            d = v;
            pos = j;
            orig = -2;
        } else if (v == d && j != pos) {
            if (orig == -2) orig = ix[pos];
            const int oj = ix[j];
            if (oj < orig) {
                pos = j;
                orig = oj;
            }
        }
    }
    // the team's argmin in every lane ((d, orig) is a strict order over distinct points: every lane ends with the same one)
    __device__ __forceinline__ void team(const int* __restrict__ ix) {
        if (orig == -2) orig = ix[pos];
        for (int m = kNnTeam / 2; m > 0; m >>= 1) {
            const float od = __shfl_xor(d, m, kNnTeam);
            const int oo = __shfl_xor(orig, m, kNnTeam);
            const int op = __shfl_xor(pos, m, kNnTeam);
            if (od < d || (od == d && oo < orig)) {
                d = od;
                orig = oo;
                pos = op;
            }
        }
    }
    // strictly closer than every unvisited point: none of them can tie with the match (at d == bound2 one could, and
    // could carry the lower index)
    __device__ __forceinline__ bool settled(float bound2) const { return d < bound2; }
    // a block that could only tie is still scanned: its point may carry the lower index
    __device__ __forceinline__ bool skip(float lb) const { return lb > d; }
};

// up to kNnCells cells of a ring cube (cell k0, k0 + kNnTeam, ...: one lane's share), each level of loads (block table,
// cell offsets, points) issued for all of them before any is consumed
template <class Tracker>
__device__ __forceinline__ void nn_cells(int k0, int ncell, int side, int ring, const int c[3], const int db[3], const int nbk[3],
                                         const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                         const float4* __restrict__ pts, const int* __restrict__ idx, const float q[3], Tracker& a) {
    int occ[kNnCells], lc[kNnCells], b[kNnCells], n[kNnCells];
#pragma unroll
    for (int i = 0; i < kNnCells; ++i) {
        const int k = k0 + i * kNnTeam;
        const int x = c[0] + k % side - ring, y = c[1] + (k / side) % side - ring, z = c[2] + k / (side * side) - ring;
        const bool in = k < ncell && x >= 0 && y >= 0 && z >= 0 && x < db[0] && y < db[1] && z < db[2];
        lc[i] = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
        occ[i] = in ? block_table[((z >> 3) * nbk[1] + (y >> 3)) * nbk[0] + (x >> 3)] : -1;
    }
    int tot = 0;
#pragma unroll
    for (int i = 0; i < kNnCells; ++i) {
        b[i] = 0;
        n[i] = 0;
        if (occ[i] >= 0) {
            const int* off = cell_off + (size_t)occ[i] * (kFitBlockCells + 1);
            b[i] = off[lc[i]];
            n[i] = off[lc[i] + 1] - b[i];
        }
        tot += n[i];
    }
    // the cells' point ranges walked as one sequence, kNnU loads in flight (the last point repeated past the end)
    for (int j = 0; j < tot; j += kNnU) {
        float4 p[kNnU];
        int at[kNnU];
#pragma unroll
        for (int u = 0; u < kNnU; ++u) {
            int v = min(j + u, tot - 1);
            int id = 0;
#pragma unroll
            for (int i = 0; i < kNnCells; ++i) {
                if (v >= 0 && v < n[i]) id = b[i] + v;
                v -= n[i];
            }
            at[u] = id;
            p[u] = pts[id];
        }
#pragma unroll
        for (int u = 0; u < kNnU; ++u) a.take(nn_l2(p[u], q), at[u], idx);
    }
}

// The nearest point of a non-empty index to q, for lane t of a team: a ends team-uniform.
//   phase 1: the cubes of radius 1 and 2 around the query cell, one cell per lane per step (the inner cells of the second
//     scanned again: both trackers are idempotent).  After the cube of radius r every unvisited point lies in a cell at
//     Chebyshev distance >= r + 1: at least the query's distance to the nearest cube face away (a small slack covers
//     binning round-off), so the team stops once its tracker is settled below that;
//   phase 2 (no point that close): square shells of 8x8x8-cell blocks; each occupied block the tracker cannot skip is
//     scanned as one contiguous range split over the lanes; after block shell r every unvisited point is at least 8r
//     cells away along some axis.
template <class Tracker>
__device__ __forceinline__ void nn_walk(const float q[3], int t, const GridHeader* __restrict__ h, const int db[3], const int nbk[3],
                                        float cell, const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                        const float4* __restrict__ fit_pts, Tracker& a) {
    const int* __restrict__ idx = a.index();
    int c[3];
    for (int k = 0; k < 3; ++k) c[k] = (int)(floorf(q[k] * h->inv_leaf[k]) - (float)h->min_b[k]);
    const float slack = 1e-4f * cell + 4e-7f * (fabsf(q[0]) + fabsf(q[1]) + fabsf(q[2]));
    int r0 = 0, rmax = 0;
    for (int k = 0; k < 3; ++k) {
        const int out = c[k] < 0 ? -c[k] : (c[k] >= db[k] ? c[k] - db[k] + 1 : 0);
        r0 = max(r0, out);
        rmax = max(rmax, max(c[k], db[k] - 1 - c[k]));
    }
    rmax = max(rmax, r0);
    // distance from the query to the nearest face of its own cell
    float face = cell;
    for (int k = 0; k < 3; ++k) {
        const float lo = (float)(c[k] + h->min_b[k]) * h->leaf[k];
        face = fminf(face, fminf(fmaxf(q[k] - lo, 0.f), fmaxf(lo + h->leaf[k] - q[k], 0.f)));
    }
    bool done = false;
    // ---- phase 1
    if (r0 <= 2) {
        for (int ring = 1; ring <= 2 && !done; ++ring) {
            const int side = 2 * ring + 1;
            const int ncell = side * side * side;
            for (int k0 = t; k0 < ncell; k0 += kNnCells * kNnTeam)
                nn_cells(k0, ncell, side, ring, c, db, nbk, block_table, cell_off, fit_pts, idx, q, a);
            a.team(idx);
            const float bound = fmaxf(0.f, face + (float)ring * cell - slack);
            done = a.settled(bound * bound) || ring >= rmax;
        }
    }
    // ---- phase 2
    if (!done) {
        int cb[3], b0 = 0, bmax = 0;
        for (int k = 0; k < 3; ++k) {
            cb[k] = c[k] >> 3;  // arithmetic shift: floor for cells left of the grid
            const int out = cb[k] < 0 ? -cb[k] : (cb[k] >= nbk[k] ? cb[k] - nbk[k] + 1 : 0);
            b0 = max(b0, out);
            bmax = max(bmax, max(cb[k], nbk[k] - 1 - cb[k]));
        }
        bmax = max(bmax, b0);
        auto visit_block = [&](int x, int y, int z) {
            const int occ = block_table[((z * nbk[1] + y) * nbk[0]) + x];
            if (occ < 0) return;
            // lower bound: per-axis cell gap between the query cell and the block's cells
            const int bx[3] = {x, y, z};
            float lb = 0.f;
            for (int k = 0; k < 3; ++k) {
                const int lo = bx[k] * 8, hi = lo + 7;
                const int gap = c[k] < lo ? lo - c[k] - 1 : (c[k] > hi ? c[k] - hi - 1 : 0);
                const float g = fmaxf(0.f, (float)gap * cell - slack);
                lb += g * g;
            }
            if (a.skip(lb)) return;  // a is team-uniform here
            const int* off = cell_off + (size_t)occ * (kFitBlockCells + 1);
            const int e = off[kFitBlockCells];
            // a block holds up to hundreds of points: kNnU loads in flight per lane, not one round trip per point
            for (int j = off[0] + t; j < e; j += kNnU * kNnTeam) {
                float4 pp[kNnU];
#pragma unroll
                for (int u = 0; u < kNnU; ++u) pp[u] = fit_pts[min(j + u * kNnTeam, e - 1)];
#pragma unroll
                for (int u = 0; u < kNnU; ++u) a.take(nn_l2(pp[u], q), min(j + u * kNnTeam, e - 1), idx);
            }
            a.team(idx);
        };
        for (int r = b0; r <= bmax; ++r) {
            const int lo2 = max(cb[2] - r, 0), hi2 = min(cb[2] + r, nbk[2] - 1);
            const int lo1 = max(cb[1] - r, 0), hi1 = min(cb[1] + r, nbk[1] - 1);
            const int lo0 = max(cb[0] - r, 0), hi0 = min(cb[0] + r, nbk[0] - 1);
            for (int z = lo2; z <= hi2; ++z)
                for (int y = lo1; y <= hi1; ++y) {
                    if (abs(z - cb[2]) == r || abs(y - cb[1]) == r) {
                        for (int x = lo0; x <= hi0; ++x) visit_block(x, y, z);
                    } else {
                        if (cb[0] - r >= 0) visit_block(cb[0] - r, y, z);
                        if (r > 0 && cb[0] + r <= nbk[0] - 1) visit_block(cb[0] + r, y, z);
                    }
                }
            const float bound = fmaxf(0.f, (float)(8 * r) * cell - slack);
            if (a.settled(bound * bound)) break;
        }
    }
}

// ------------------------------------------------------------------------------------------------ k nearest
// The k nearest points of a cloud's own index to q, for lane t of a team: the walk of k_sor_knn (3x3x3 cube, ring 2, block
// shells, the same bound) with (d2, index) keys, for k_ground_normals (ground.hip).  Every lane ends with the C smallest
// keys it saw (C >= k), the team's k smallest among them; knn_next then hands them out in ascending order.
// k_gicp_cov (gicp.hip) keeps the copy of this walk written out in its body: called through this function it compiled to
// 125 VGPRs instead of 96 (C = 20) and 174 instead of 121 (C = 32), a wave less per SIMD.
constexpr unsigned long long kKnnNone = ~0ull;

// The C smallest keys one lane has seen, ascending (registers; branch-free min/max cascade as TopK of front_end.hip);
// a key is (d2 bits << 32 | original index), so the (d2, index) order rule is the keys' order
template <int C>
struct KnnList {
    unsigned long long v[C];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < C; ++j) v[j] = kKnnNone;
    }
    __device__ __forceinline__ void insert(unsigned long long d) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const unsigned long long lo = v[j] < d ? v[j] : d;
            d = v[j] < d ? d : v[j];
            v[j] = lo;
        }
    }
    // keys whose distance is strictly below b2
    __device__ __forceinline__ int count_lt(float b2) const {
        int n = 0;
#pragma unroll
        for (int j = 0; j < C; ++j) n += (v[j] != kKnnNone && __uint_as_float((unsigned)(v[j] >> 32)) < b2) ? 1 : 0;
        return n;
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int j = 0; j < C - 1; ++j) v[j] = v[j + 1];
        v[C - 1] = kKnnNone;
    }
};

__device__ __forceinline__ int knn_team_sum(int v) {
    for (int m = kNnTeam / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kNnTeam);
    return v;
}

// candidate j of the index: its key enters the lane's list when it can be among the C smallest
template <int C>
__device__ __forceinline__ void knn_take(KnnList<C>& top, const float4* __restrict__ ix_pts, const int* __restrict__ ix_idx, int j,
                                     const float q[3]) {
    const float d = nn_l2(ix_pts[j], q);
    const unsigned hi = __float_as_uint(d);
    if (hi > (unsigned)(top.v[C - 1] >> 32)) return;  // d2 >= 0: the bits order as the values
    top.insert(((unsigned long long)hi << 32) | (unsigned)ix_idx[j]);
}

template <int C>
__device__ __forceinline__ void knn_walk(const float q[3], int t, int k, const GridHeader* __restrict__ h, const int db[3], const int nbk[3],
                                         float cell, const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                         const float4* __restrict__ ix_pts, const int* __restrict__ ix_idx, KnnList<C>& top) {
    top.init();
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = (int)(floorf(q[a] * h->inv_leaf[a]) - (float)h->min_b[a]);
    const float slack = 1e-4f * cell + 4e-7f * (fabsf(q[0]) + fabsf(q[1]) + fabsf(q[2]));
    int rmax = 0;
    for (int a = 0; a < 3; ++a) rmax = max(rmax, max(c[a], db[a] - 1 - c[a]));
    bool done = false;
    for (int ring = 1; ring <= 2 && !done; ++ring) {
        const int side = 2 * ring + 1, total = side * side * side;
        for (int kk = t; kk < total; kk += kNnTeam) {
            const int dx = kk % side - ring, dy = (kk / side) % side - ring, dz = kk / (side * side) - ring;
            if (ring == 2 && abs(dx) < 2 && abs(dy) < 2 && abs(dz) < 2) continue;
            const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
            if (x < 0 || y < 0 || z < 0 || x >= db[0] || y >= db[1] || z >= db[2]) continue;
            const int occ = block_table[(((z >> 3) * nbk[1] + (y >> 3)) * nbk[0]) + (x >> 3)];
            if (occ < 0) continue;
            const int l = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
            const int* off = cell_off + (size_t)occ * (kFitBlockCells + 1);
            const int e = off[l + 1];
            for (int j = off[l]; j < e; ++j) knn_take<C>(top, ix_pts, ix_idx, j, q);
        }
        // every unvisited point is at least `bound` away: k visited candidates strictly closer end the search, and
        // no unvisited point can tie with any of them
        const float bound = fmaxf(0.f, (float)ring * cell - slack);
        done = knn_team_sum(top.count_lt(bound * bound)) >= k || ring >= rmax;
    }
    if (!done) {
        int cb[3], bmax = 0;
        for (int a = 0; a < 3; ++a) {
            cb[a] = c[a] >> 3;
            bmax = max(bmax, max(cb[a], nbk[a] - 1 - cb[a]));
        }
        top.init();  // fresh lists: every point of every visited block exactly once
        for (int r = 0; r <= bmax; ++r) {
            const int lo2 = max(cb[2] - r, 0), hi2 = min(cb[2] + r, nbk[2] - 1);
            const int lo1 = max(cb[1] - r, 0), hi1 = min(cb[1] + r, nbk[1] - 1);
            const int lo0 = max(cb[0] - r, 0), hi0 = min(cb[0] + r, nbk[0] - 1);
            // every block of the cube is tested and the interior skipped: enumerating only the faces (as nn_walk does,
            // three inlined scans) took 130 VGPRs instead of 96 and the target covariances 1.34 ms instead of 1.10
            for (int z = lo2; z <= hi2; ++z)
                for (int y = lo1; y <= hi1; ++y)
                    for (int x = lo0; x <= hi0; ++x) {
                        if (abs(z - cb[2]) != r && abs(y - cb[1]) != r && abs(x - cb[0]) != r) continue;
                        const int occ = block_table[((z * nbk[1] + y) * nbk[0]) + x];
                        if (occ < 0) continue;
                        const int* off = cell_off + (size_t)occ * (kFitBlockCells + 1);
                        const int e = off[kFitBlockCells];
                        for (int j = off[0] + t; j < e; j += kNnTeam) knn_take<C>(top, ix_pts, ix_idx, j, q);
                    }
            const float bound = fmaxf(0.f, (float)(8 * r) * cell - slack);
            if (knn_team_sum(top.count_lt(bound * bound)) >= k) break;
        }
    }
}

// the team's next smallest key in every lane (keys are distinct), kKnnNone once the lists are empty
template <int C>
__device__ __forceinline__ unsigned long long knn_next(KnnList<C>& top) {
    unsigned long long m = top.v[0];
    for (int off = kNnTeam / 2; off > 0; off >>= 1) {
        const unsigned long long om = __shfl_xor(m, off, kNnTeam);
        m = om < m ? om : m;
    }
    if (m != kKnnNone && top.v[0] == m) top.pop();
    return m;
}

}  // namespace ndt
