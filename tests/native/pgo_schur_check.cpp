// The two identities of the pose graph's direct solve on the host (xchu_slam_amd/csrc/ndt_pgo_schur.h: the text
// k_pgo_schur runs), on a seeded 12-node chain with three loops (one nested in another, one given reversed) and two
// position factors (one on node 0): d = 24.
//   1. pgo_schur_block from the prefix table C against B B^T formed densely, B = Kw (sum_s s E_node_s) L P.
//   2. Woodbury's step (u = L P g, b, z = S^-1 b, f, y = g - P^T suffix(f)) against a dense solve of (I + B^T B) y = g.
// Both sides are the same f64 sums in different orders; each line prints the largest difference relative to the largest
// entry, and the exit status is 1 when one exceeds 1e-12.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../xchu_slam_amd/csrc/ndt_pgo_schur.h"

using namespace ndt;

static unsigned long long rng_state = 0x9e3779b97f4a7c15ULL;
static double uniform() {  // splitmix64, (-1, 1)
    unsigned long long z = (rng_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}

// Solves A x = b in place (Gaussian elimination with partial pivoting), A n x n row-major
static void solve(std::vector<double> A, std::vector<double>& b, int n) {
    for (int k = 0; k < n; ++k) {
        int piv = k;
        for (int r = k + 1; r < n; ++r)
            if (std::fabs(A[r * n + k]) > std::fabs(A[piv * n + k])) piv = r;
        for (int c = 0; c < n; ++c) std::swap(A[k * n + c], A[piv * n + c]);
        std::swap(b[k], b[piv]);
        for (int r = k + 1; r < n; ++r) {
            const double f = A[r * n + k] / A[k * n + k];
            for (int c = k; c < n; ++c) A[r * n + c] -= f * A[k * n + c];
            b[r] -= f * b[k];
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        for (int c = k + 1; c < n; ++c) b[k] -= A[k * n + c] * b[c];
        b[k] /= A[k * n + k];
    }
}

int main() {
    const int n = 12, m = 3, np = 2, N = 6 * n, d = 6 * m + 3 * np;
    const int li[m] = {1, 3, 10}, lj[m] = {9, 6, 2}, pnode[np] = {0, 7};
    // P_t: a rotation-sized block scaled like Ad(X_t) Jr diag(sigma) (a lever arm of tens of metres below the diagonal)
    std::vector<double> P(36 * n), kw(6 * d), g(N);
    for (int t = 0; t < n; ++t)
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                const double lever = (r >= 3 && c < 3) ? 20.0 : 1.0, sigma = c < 3 ? 1e-3 : 1e-2;
                P[36 * t + 6 * r + c] = (r < 3 && c >= 3) ? 0.0 : lever * sigma * uniform();
            }
    for (int i = 0; i < 6 * d; ++i) kw[i] = 30.0 * uniform();
    for (int i = 0; i < N; ++i) g[i] = uniform();
    // the table: C_k = sum_{t <= k} P_t P_t^T
    std::vector<double> C(36 * n, 0.0);
    for (int t = 0; t < n; ++t)
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                double acc = t ? C[36 * (t - 1) + 6 * r + c] : 0.0;
                for (int k = 0; k < 6; ++k) acc += P[36 * t + 6 * r + k] * P[36 * t + 6 * c + k];
                C[36 * t + 6 * r + c] = acc;
            }
    // B densely: row block a = Kw_a (sum_s s E_node_s) L P; (E_k L P)'s column block t is P_t for t <= k
    std::vector<double> B((size_t)d * N, 0.0);
    for (int f = 0; f < m + np; ++f) {
        const PgoFactorRef a = pgo_factor_ref(f, m, li, lj, pnode);
        for (int side = 0; side < 2; ++side) {
            const int node = side ? a.minus : a.plus;
            if (node < 0) continue;
            const double sgn = side ? -1.0 : 1.0;
            for (int t = 0; t <= node; ++t)
                for (int r = 0; r < a.nr; ++r)
                    for (int c = 0; c < 6; ++c) {
                        double acc = 0.0;
                        for (int k = 0; k < 6; ++k) acc += kw[6 * (a.row + r) + k] * P[36 * t + 6 * k + c];
                        B[(size_t)(a.row + r) * N + 6 * t + c] += sgn * acc;
                    }
        }
    }
    // 1. the blocks
    std::vector<double> S((size_t)d * d, 0.0);
    double worst = 0.0, scale = 0.0;
    for (int fa = 0; fa < m + np; ++fa)
        for (int fb = 0; fb < m + np; ++fb) {
            const PgoFactorRef a = pgo_factor_ref(fa, m, li, lj, pnode), b = pgo_factor_ref(fb, m, li, lj, pnode);
            pgo_schur_block(C.data(), kw.data(), a, b, S.data() + (size_t)a.row * d + b.row, (size_t)d);
        }
    for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c) {
            double acc = 0.0;
            for (int k = 0; k < N; ++k) acc += B[(size_t)r * N + k] * B[(size_t)c * N + k];
            scale = std::fmax(scale, std::fabs(acc));
            worst = std::fmax(worst, std::fabs(acc - S[(size_t)r * d + c]));
        }
    const double e1 = worst / scale;
    std::printf("schur_block %.3e (largest entry %.3e)\n", e1, scale);
    // 2. Woodbury's step against the dense solve
    std::vector<double> H((size_t)N * N, 0.0), y = g;
    for (int r = 0; r < N; ++r)
        for (int c = 0; c < N; ++c) {
            double acc = r == c ? 1.0 : 0.0;
            for (int k = 0; k < d; ++k) acc += B[(size_t)k * N + r] * B[(size_t)k * N + c];
            H[(size_t)r * N + c] = acc;
        }
    solve(H, y, N);
    std::vector<double> u(N), b(d), f(N, 0.0), yw(N);
    for (int k = 0; k < n; ++k)  // u = L P g
        for (int r = 0; r < 6; ++r) {
            double acc = k ? u[6 * (k - 1) + r] : 0.0;
            for (int c = 0; c < 6; ++c) acc += P[36 * k + 6 * r + c] * g[6 * k + c];
            u[6 * k + r] = acc;
        }
    for (int fa = 0; fa < m + np; ++fa) {  // b_a = Kw_a sum_s s u_node_s
        const PgoFactorRef a = pgo_factor_ref(fa, m, li, lj, pnode);
        for (int r = 0; r < a.nr; ++r) {
            double acc = 0.0;
            for (int c = 0; c < 6; ++c) acc += kw[6 * (a.row + r) + c] * (u[6 * a.plus + c] - (a.minus >= 0 ? u[6 * a.minus + c] : 0.0));
            b[a.row + r] = acc;
        }
    }
    for (int r = 0; r < d; ++r) S[(size_t)r * d + r] += 1.0;
    solve(S, b, d);  // z
    for (int fa = 0; fa < m + np; ++fa) {  // f_k = sum_{a contains k} s Kw_a^T z_a
        const PgoFactorRef a = pgo_factor_ref(fa, m, li, lj, pnode);
        for (int c = 0; c < 6; ++c) {
            double acc = 0.0;
            for (int r = 0; r < a.nr; ++r) acc += kw[6 * (a.row + r) + c] * b[a.row + r];
            f[6 * a.plus + c] += acc;
            if (a.minus >= 0) f[6 * a.minus + c] -= acc;
        }
    }
    double suf[6] = {0, 0, 0, 0, 0, 0};
    for (int k = n - 1; k >= 0; --k) {  // y = g - P^T suffix(f)
        for (int c = 0; c < 6; ++c) suf[c] += f[6 * k + c];
        for (int c = 0; c < 6; ++c) {
            double acc = 0.0;
            for (int r = 0; r < 6; ++r) acc += P[36 * k + 6 * r + c] * suf[r];
            yw[6 * k + c] = g[6 * k + c] - acc;
        }
    }
    worst = scale = 0.0;
    for (int i = 0; i < N; ++i) {
        scale = std::fmax(scale, std::fabs(y[i]));
        worst = std::fmax(worst, std::fabs(y[i] - yw[i]));
    }
    const double e2 = worst / scale;
    std::printf("woodbury_step %.3e (largest entry %.3e)\n", e2, scale);
    return e1 <= 1e-12 && e2 <= 1e-12 ? 0 : 1;
}
