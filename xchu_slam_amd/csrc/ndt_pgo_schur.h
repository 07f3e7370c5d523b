// ndt_pgo_schur.h — one block of the direct solve's loop-space matrix S = I + B B^T (DESIGN.md §2 "Pose graph", direct
// solve), as the device builds it (posegraph_direct.hip: k_pgo_schur) and as tests/native/pgo_schur_check.cpp checks it
// on the host against B B^T formed densely.
//
// A factor a owns nr rows of B (6: a between factor, 3: a position factor):  B_a = Kw_a (sum_s s E_node_s) L P, with
// s = +1 at `plus` (a between factor's j, a position factor's node) and s = -1 at `minus` (a between factor's i; none,
// -1, for a position factor).  Because (L P P^T L^T)_{kl} = C_min(k,l), C_k = sum_{t <= k} P_t P_t^T, the block is
//     (B B^T)_{ab} = Kw_a Ov(a, b) Kw_b^T,   Ov(a, b) = sum_{s in a} sum_{s' in b} s s' C_min(node_s, node_s'):
// four (two, one) entries of the table, never a sum over the nodes between two factors.
// Host/device text (NDT_HD): a host compiler reads it without the HIP headers.
#pragma once
#include <stddef.h>
#include "ndt_linalg.h"

namespace ndt {

constexpr int kPgoDirectTile = 32;       // tile width of the blocked Cholesky factorisation
constexpr int kPgoDirectMaxDim = 8192;   // largest d = 6 m + 3 np: (d + 1) d doubles stay near 512 MB
constexpr double kPgoPivotMin = 1.0 - 1e-6;  // every eigenvalue of S is >= 1, so is every pivot

struct PgoFactorRef {
    int row;    // first row of B (and of S)
    int nr;     // rows: 6 or 3
    int plus;   // node with s = +1
    int minus;  // node with s = -1, or -1
};

// Factor f of a graph with m between factors (li, lj) and then its position factors by slot (pnode[slot])
NDT_HD PgoFactorRef pgo_factor_ref(int f, int m, const int* li, const int* lj, const int* pnode) {
    if (f < m) return PgoFactorRef{6 * f, 6, lj[f], li[f]};
    return PgoFactorRef{6 * m + 3 * (f - m), 3, pnode[f - m], -1};
}

// Ov(a, b) from the table C ([n][36], row-major 6 x 6 per node): (C_min(a+,b+) - C_min(a+,b-)) - (C_min(a-,b+) - C_min(a-,b-)),
// each difference taken first, so that two overlapping intervals lose the route's common prefix before anything else.
NDT_HD void pgo_overlap(const double* C, const PgoFactorRef& a, const PgoFactorRef& b, double* Ov) {
    auto at = [C](int k, int l) { return C + 36 * (size_t)(k < l ? k : l); };
    const double* pp = at(a.plus, b.plus);
    for (int i = 0; i < 36; ++i) Ov[i] = pp[i];
    if (b.minus >= 0) {
        const double* pm = at(a.plus, b.minus);
        for (int i = 0; i < 36; ++i) Ov[i] = Ov[i] - pm[i];
    }
    if (a.minus >= 0) {
        const double* mp = at(a.minus, b.plus);
        if (b.minus >= 0) {
            const double* mm = at(a.minus, b.minus);
            for (int i = 0; i < 36; ++i) Ov[i] = Ov[i] - (mp[i] - mm[i]);
        } else {
            for (int i = 0; i < 36; ++i) Ov[i] = Ov[i] - mp[i];
        }
    }
}

// out[r * ld + c] = (Kw_a Ov(a, b) Kw_b^T)_{rc}, r < a.nr, c < b.nr; kw holds one row of 6 per row of B.  Sums run over
// the inner index in ascending order.
NDT_HD void pgo_schur_block(const double* C, const double* kw, const PgoFactorRef& a, const PgoFactorRef& b,
                                                double* out, size_t ld) {
    double Ov[36];
    pgo_overlap(C, a, b, Ov);
    for (int r = 0; r < a.nr; ++r) {
        const double* ka = kw + 6 * (size_t)(a.row + r);
        double t[6];
        for (int c = 0; c < 6; ++c) {
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc = acc + ka[k] * Ov[6 * k + c];
            t[c] = acc;
        }
        for (int c = 0; c < b.nr; ++c) {
            const double* kb = kw + 6 * (size_t)(b.row + c);
            double acc = 0.0;
            for (int k = 0; k < 6; ++k) acc = acc + t[k] * kb[k];
            out[r * ld + c] = acc;
        }
    }
}

}  // namespace ndt
