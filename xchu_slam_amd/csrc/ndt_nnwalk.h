// ndt_nnwalk.h — the exact nearest-neighbour walk of one 16-lane team over an NNIndex, with the argmin and the
// lowest-original-index tie rule (device only).  Shared by k_icp_pass (icp.hip) and k_gicp_pairs (gicp.hip).
//
// The walk is k_fitness's (voxel_build.hip: 3x3x3 cube, 5x5x5 cube, block shells) tracking the argmin beside the
// minimum; equal f32 distances go to the lowest index in the caller's order (the index build carries that index as a
// fifth word beside the sorted points).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "ndt_types.h"
#include "ndt_icp.h"

namespace ndt {

constexpr int kIcpU = 8;      // point loads in flight per lane
constexpr int kIcpCells = 2;  // ring-cube cells per lane per step

// running argmin of one lane: squared distance, position in the index, original target index (-2: not loaded yet)
struct Arg {
    float d;
    int pos, orig;
};

// FLANN L2_Simple in f32, as l2_simple of voxel_build.hip
__device__ __forceinline__ float icp_l2(const float4 t, const float q[3]) {
    float d = 0.f, u;
    u = t.x - q[0]; d += u * u;
    u = t.y - q[1]; d += u * u;
    u = t.z - q[2]; d += u * u;
    return d;
}

// candidate j at distance d; a tie goes to the lower original index (loaded only then); a repeated j changes nothing
__device__ __forceinline__ void arg_take(Arg& a, float d, int j, const int* __restrict__ idx) {
    if (d < a.d) {
        a.d = d;
        a.pos = j;
        a.orig = -2;
    } else if (d == a.d && j != a.pos) {
        if (a.orig == -2) a.orig = idx[a.pos];
        const int oj = idx[j];
        if (oj < a.orig) {
            a.pos = j;
            a.orig = oj;
        }
    }
}

// the team's argmin in every lane ((d, orig) is a strict order over distinct points: every lane ends with the same one)
__device__ __forceinline__ void arg_team(Arg& a, const int* __restrict__ idx) {
    if (a.orig == -2) a.orig = idx[a.pos];
    for (int m = kIcpTeam / 2; m > 0; m >>= 1) {
        const float od = __shfl_xor(a.d, m, kIcpTeam);
        const int oo = __shfl_xor(a.orig, m, kIcpTeam);
        const int op = __shfl_xor(a.pos, m, kIcpTeam);
        if (od < a.d || (od == a.d && oo < a.orig)) {
            a.d = od;
            a.orig = oo;
            a.pos = op;
        }
    }
}

// up to kIcpCells cells of a ring cube (cell k0, k0 + kIcpTeam, ...: one lane's share), as cells_min of voxel_build.hip
__device__ __forceinline__ void cells_arg(int k0, int ncell, int side, int ring, const int c[3], const int db[3], const int nbk[3],
                                          const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                          const float4* __restrict__ pts, const int* __restrict__ idx, const float q[3], Arg& a) {
    int occ[kIcpCells], lc[kIcpCells], b[kIcpCells], n[kIcpCells];
#pragma unroll
    for (int i = 0; i < kIcpCells; ++i) {
        const int k = k0 + i * kIcpTeam;
        const int x = c[0] + k % side - ring, y = c[1] + (k / side) % side - ring, z = c[2] + k / (side * side) - ring;
        const bool in = k < ncell && x >= 0 && y >= 0 && z >= 0 && x < db[0] && y < db[1] && z < db[2];
        lc[i] = ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
        occ[i] = in ? block_table[((z >> 3) * nbk[1] + (y >> 3)) * nbk[0] + (x >> 3)] : -1;
    }
    int tot = 0;
#pragma unroll
    for (int i = 0; i < kIcpCells; ++i) {
        b[i] = 0;
        n[i] = 0;
        if (occ[i] >= 0) {
            const int* off = cell_off + (size_t)occ[i] * (kFitBlockCells + 1);
            b[i] = off[lc[i]];
            n[i] = off[lc[i] + 1] - b[i];
        }
        tot += n[i];
    }
    for (int j = 0; j < tot; j += kIcpU) {
        float4 p[kIcpU];
        int at[kIcpU];
#pragma unroll
        for (int u = 0; u < kIcpU; ++u) {
            int v = min(j + u, tot - 1);
            int id = 0;
#pragma unroll
            for (int i = 0; i < kIcpCells; ++i) {
                if (v >= 0 && v < n[i]) id = b[i] + v;
                v -= n[i];
            }
            at[u] = id;
            p[u] = pts[id];
        }
#pragma unroll
        for (int u = 0; u < kIcpU; ++u) arg_take(a, icp_l2(p[u], q), at[u], idx);
    }
}

// The nearest point of a non-empty index to q, for lane t of a team: a ends team-uniform (pos -1: none found).
__device__ __forceinline__ void nn_walk(const float q[3], int t, const GridHeader* __restrict__ h, const int db[3], const int nbk[3],
                                        float cell, const int* __restrict__ block_table, const int* __restrict__ cell_off,
                                        const float4* __restrict__ fit_pts, const int* __restrict__ fit_idx, Arg& a) {
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
    float face = cell;
    for (int k = 0; k < 3; ++k) {
        const float lo = (float)(c[k] + h->min_b[k]) * h->leaf[k];
        face = fminf(face, fminf(fmaxf(q[k] - lo, 0.f), fmaxf(lo + h->leaf[k] - q[k], 0.f)));
    }
    bool done = false;
    // ---- phase 1: the cubes of radius 1 and 2 around the query cell, one cell per lane per step
    if (r0 <= 2) {
        for (int ring = 1; ring <= 2 && !done; ++ring) {
            const int side = 2 * ring + 1;
            const int ncell = side * side * side;
            for (int k0 = t; k0 < ncell; k0 += kIcpCells * kIcpTeam)
                cells_arg(k0, ncell, side, ring, c, db, nbk, block_table, cell_off, fit_pts, fit_idx, q, a);
            arg_team(a, fit_idx);
            // every unvisited point is at least `bound` away; strictly closer than that and no unvisited point can
            // tie with the match
            const float bound = fmaxf(0.f, face + (float)ring * cell - slack);
            done = a.d < bound * bound || ring >= rmax;
        }
    }
    // ---- phase 2: block shells, each candidate block's points split over the team
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
            const int bx[3] = {x, y, z};
            float lb = 0.f;
            for (int k = 0; k < 3; ++k) {
                const int lo = bx[k] * 8, hi = lo + 7;
                const int gap = c[k] < lo ? lo - c[k] - 1 : (c[k] > hi ? c[k] - hi - 1 : 0);
                const float g = fmaxf(0.f, (float)gap * cell - slack);
                lb += g * g;
            }
            if (lb > a.d) return;  // a is team-uniform here; a block that could only tie is still scanned
            const int* off = cell_off + (size_t)occ * (kFitBlockCells + 1);
            const int e = off[kFitBlockCells];
            for (int j = off[0] + t; j < e; j += kIcpU * kIcpTeam) {
                float4 pp[kIcpU];
#pragma unroll
                for (int u = 0; u < kIcpU; ++u) pp[u] = fit_pts[min(j + u * kIcpTeam, e - 1)];
#pragma unroll
                for (int u = 0; u < kIcpU; ++u) arg_take(a, icp_l2(pp[u], q), min(j + u * kIcpTeam, e - 1), fit_idx);
            }
            arg_team(a, fit_idx);
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
            if (a.d < bound * bound) break;
        }
    }
}

}  // namespace ndt
