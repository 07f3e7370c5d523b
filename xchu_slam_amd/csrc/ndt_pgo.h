// ndt_pgo.h — the pose-graph optimiser (pgo_node's GTSAM back end restated as a batch problem, DESIGN.md §2 "Pose
// graph"): the device layout of a graph and the SE(3) arithmetic that k_pgo_optimize (posegraph.hip) is made of.
//
// A pose is 12 doubles: R row-major, then t.  Tangent vectors are [wx wy wz vx vy vz] (GTSAM's Pose3 order), the
// retraction is X <- X Exp(d), a between residual is e = Log(Z^-1 Xi^-1 Xj) with the full SE(3) logarithm.
// Every coefficient function of |w| switches to its power series below kPgoSeries, so the logarithm and both Jacobians
// are finite at |w| == 0 exactly (every odometry residual starts there).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ndt_hip.h"

namespace ndt {

constexpr int kPgoBlock = 512;          // the one workgroup of k_pgo_optimize
constexpr int kPgoWaves = kPgoBlock / 64;
constexpr double kPgoSeries = 0.2;      // |w| below which the series are used (six terms: truncation < 1e-17 relative)
constexpr double kPgoPiMargin = 1e-6;   // residual rotations closer to pi than this are rejected
constexpr int kPgoMaxIter = 10000;      // bound of ndt_pgo_params.max_iter / cg_max_iter

// ndt_pgo_optimize's status word
enum PgoStatus : int { kPgoOk = 0, kPgoNearPi = 1, kPgoNotFinite = 2 };

struct PgoOut {
    int status;         // PgoStatus
    int bad;            // kPgoNearPi: the factor (chain factor k < n, loop edge k - n)
    int iterations;
    int converged;
    int cg_iterations;  // summed over the outer iterations
    int pad;
    double cost0, cost, max_step;
};

// One graph on the device.  Chain factor k is the prior (k == 0, measurement = the first pose as given) or the odometry
// edge (k - 1, k); loop edges are the ndt_pgo_add_between ones.  ent[off[k] .. off[k + 1]) lists node k's loop edges as
// 2 * edge + side (side 1: the node is the edge's j).  Position factors are the ndt_pgo_add_position ones (residual
// t_k - z, no logarithm), stored by node and within a node in insertion order (the host sorts them and puts the weights
// back in insertion order): node k's are the slots poff[k] .. poff[k + 1].  They share two pointers, not one per array:
// the kernel already runs out of registers.
struct PgoGraph {
    int n, m, np;
    double* X;            // [n][12] the estimate
    double* Xprev;        // [n][12] the estimate before the last step
    const double* Zc;     // [n][12]
    const int* li;        // [m]
    const int* lj;        // [m]
    const double* Zl;     // [m][12]
    const double* lvar;   // [m][6]
    const double* lk;     // [m] robust k (0: Gaussian)
    const int* off;       // [n + 1]
    const int* ent;       // [2 m]
    double* Jc;           // [n][18] Jr(e_k): its rotation block, then its lower-left block
    double* rc;           // [n][6] whitened chain residuals
    double* N;            // [m][36] w K^T K, K = S Jr^-1(e) Ad(Xj^-1)
    double* bv;           // [m][6]  w K^T S e
    double* dl;           // [m][6]  per-edge product of the matrix-vector step
    double* w;            // [m]     robust weights
    const int* poff;      // [n + 1], then [np] each position factor's node
    double* pf;           // [np][7] measured xyz, variances, robust k (0: Gaussian); then [np][7] w / var, w (t_k - z) / var, w
    double* z;            // [n][6]  prefix sums (world frame)
    double* tmp;          // [n][6]  a scan's per-thread running sums
    double* y;            // [n][6]  CG iterate, residual, direction, product
    double* r;
    double* p;
    double* hp;
    ndt_pgo_record* hist; // [max_iter + 1]
    PgoOut* out;
};

struct PgoArgs {
    int max_iter, cg_max_iter;
    double step_eps, cg_rtol;
    double sig_prior[6], sig_odom[6];   // standard deviations
};

// The direct loop-space solve (posegraph_direct.hip).  d = 6 m + 3 np rows of B: between factor q owns rows 6 q .. 6 q + 5,
// the position factor in slot q rows 6 m + 3 q .. + 2.  S is dp x dp (d rounded up to whole tiles, the padding an identity),
// lower triangle, row-major with leading dimension dp; row dp carries b, then the forward solve, then z = S^-1 b.
struct PgoDirectState {
    int status;         // PgoStatus
    int bad;            // kPgoNearPi: the factor, as PgoOut's
    int iterations;
    int converged;
    int done;           // the host enqueues no further iteration
    int pivot_bad;      // a pivot of the factorisation was not finite or below kPgoPivotMin
    double cost0, cost, max_step;
};

struct PgoDirect {
    int d, dp;
    double* kw;           // [d][6]  one row of Kw per row of B
    double* C;            // [n][36] prefix sums of P_t P_t^T
    double* S;            // [dp + 1][dp]
    PgoDirectState* st;
};

// ------------------------------------------------------------------------------------------------ 3 x 3 helpers
__host__ __device__ inline void m3_mul(const double* A, const double* B, double* C) {  // C = A B
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__host__ __device__ inline void m3_tmul(const double* A, const double* B, double* C) {  // C = A^T B
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__host__ __device__ inline void m3_vec(const double* A, const double* v, double* o) {  // o = A v
    for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
__host__ __device__ inline void m3_tvec(const double* A, const double* v, double* o) {  // o = A^T v
    for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
__host__ __device__ inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ inline void hat3(const double* w, double* W) {
    W[0] = 0.0, W[1] = -w[2], W[2] = w[1];
    W[3] = w[2], W[4] = 0.0, W[5] = -w[0];
    W[6] = -w[1], W[7] = w[0], W[8] = 0.0;
}
// M = I + a W + b W^2, W = hat(w)
__host__ __device__ inline void so3_poly(const double* w, double a, double b, double* M) {
    double W[9], W2[9];
    hat3(w, W);
    m3_mul(W, W, W2);
    for (int i = 0; i < 9; ++i) M[i] = a * W[i] + b * W2[i];
    M[0] += 1.0, M[4] += 1.0, M[8] += 1.0;
}

// ------------------------------------------------------------------------------------------------ poses
// C = A^-1 B
__host__ __device__ inline void pose_inv_mul(const double* A, const double* B, double* C) {
    m3_tmul(A, B, C);
    const double d[3] = {B[9] - A[9], B[10] - A[10], B[11] - A[11]};
    m3_tvec(A, d, C + 9);
}
// C = A B
__host__ __device__ inline void pose_mul(const double* A, const double* B, double* C) {
    m3_mul(A, B, C);
    double t[3];
    m3_vec(A, B + 9, t);
    for (int i = 0; i < 3; ++i) C[9 + i] = t[i] + A[9 + i];
}
// o = Ad(X) v = [R w; t x (R w) + R v]
__host__ __device__ inline void ad_vec(const double* X, const double* v, double* o) {
    double c[3];
    m3_vec(X, v, o);
    m3_vec(X, v + 3, o + 3);
    cross3(X + 9, o, c);
    for (int i = 0; i < 3; ++i) o[3 + i] += c[i];
}
// o = Ad(X^-1) v = [R^T w; R^T (v - t x w)]
__host__ __device__ inline void ad_inv_vec(const double* X, const double* v, double* o) {
    double c[3];
    cross3(X + 9, v, c);
    const double d[3] = {v[3] - c[0], v[4] - c[1], v[5] - c[2]};
    m3_tvec(X, v, o);
    m3_tvec(X, d, o + 3);
}
// o = Ad(X)^T v = [R^T (a - t x b); R^T b]
__host__ __device__ inline void ad_t_vec(const double* X, const double* v, double* o) {
    double c[3];
    cross3(X + 9, v + 3, c);
    const double d[3] = {v[0] - c[0], v[1] - c[1], v[2] - c[2]};
    m3_tvec(X, d, o);
    m3_tvec(X, v + 3, o + 3);
}

// ------------------------------------------------------------------------------------------------ coefficients
struct PgoCoef {
    double A;  // sin(th) / th
    double B;  // (1 - cos th) / th^2
    double C;  // (th - sin th) / th^3
    double D;  // (1 - th/2 cot(th/2)) / th^2
    double E;  // (th^2/2 + cos th - 1) / th^4
    double F;  // (2 th + th cos th - 3 sin th) / (2 th^5)
};

__host__ __device__ inline double pgo_horner(double t, double c0, double c1, double c2, double c3, double c4, double c5) {
    return ((((c5 * t + c4) * t + c3) * t + c2) * t + c1) * t + c0;
}

__host__ __device__ inline PgoCoef pgo_coef(double th) {
    PgoCoef k;
    const double t = th * th;
    if (th < kPgoSeries) {
        k.A = pgo_horner(t, 1.0, -1.0 / 6, 1.0 / 120, -1.0 / 5040, 1.0 / 362880, -1.0 / 39916800);
        k.B = pgo_horner(t, 1.0 / 2, -1.0 / 24, 1.0 / 720, -1.0 / 40320, 1.0 / 3628800, -1.0 / 479001600);
        k.C = pgo_horner(t, 1.0 / 6, -1.0 / 120, 1.0 / 5040, -1.0 / 362880, 1.0 / 39916800, -1.0 / 6227020800.0);
        k.D = pgo_horner(t, 1.0 / 12, 1.0 / 720, 1.0 / 30240, 1.0 / 1209600, 1.0 / 47900160, 691.0 / 1307674368000.0);
        k.E = pgo_horner(t, 1.0 / 24, -1.0 / 720, 1.0 / 40320, -1.0 / 3628800, 1.0 / 479001600, -1.0 / 87178291200.0);
        k.F = pgo_horner(t, 1.0 / 120, -2.0 / 5040, 3.0 / 362880, -4.0 / 39916800, 5.0 / 6227020800.0, -6.0 / 1307674368000.0);
    } else {
        const double s = sin(th), c = cos(th), h = 0.5 * th;
        k.A = s / th;
        k.B = (1.0 - c) / t;
        k.C = (th - s) / (t * th);
        k.D = (1.0 - h * cos(h) / sin(h)) / t;
        k.E = (0.5 * t + c - 1.0) / (t * t);
        k.F = (2.0 * th + th * c - 3.0 * s) / (2.0 * t * t * th);
    }
    return k;
}

__host__ __device__ inline double norm3(const double* v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// X = Exp(d)
__host__ __device__ inline void pgo_exp(const double* d, double* X) {
    const PgoCoef k = pgo_coef(norm3(d));
    double V[9];
    so3_poly(d, k.A, k.B, X);
    so3_poly(d, k.B, k.C, V);
    m3_vec(V, d + 3, X + 9);
}

// e = Log(X); false when the rotation is within kPgoPiMargin of pi (e is then not written)
__host__ __device__ inline bool pgo_log(const double* X, double* e) {
    const double a[3] = {0.5 * (X[7] - X[5]), 0.5 * (X[2] - X[6]), 0.5 * (X[3] - X[1])};
    const double s = norm3(a), c = 0.5 * (X[0] + X[4] + X[8] - 1.0);
    const double th = atan2(s, c);
    if (!(th <= 3.14159265358979323846 - kPgoPiMargin)) return false;  // a NaN lands here too
    const double f = th < kPgoSeries ? 1.0 / pgo_coef(th).A : th / s;
    for (int i = 0; i < 3; ++i) e[i] = a[i] * f;
    double Vi[9];
    so3_poly(e, -0.5, pgo_coef(norm3(e)).D, Vi);
    m3_vec(Vi, X + 9, e + 3);
    return true;
}

// The lower-left block of Jr(e) (GTSAM's computeQforExpmapDerivative: Barfoot's Q at -e)
__host__ __device__ inline void pgo_q_right(const double* e, const PgoCoef& k, double* Q) {
    double W[9], V[9], WV[9], VW[9], WVW[9], t1[9], t2[9];
    hat3(e, W);
    hat3(e + 3, V);
    m3_mul(W, V, WV);
    m3_mul(V, W, VW);
    m3_mul(WV, W, WVW);
    for (int i = 0; i < 9; ++i) Q[i] = -0.5 * V[i] + k.C * (WV[i] + VW[i] - WVW[i]);
    m3_mul(W, WV, t1);
    m3_mul(VW, W, t2);
    for (int i = 0; i < 9; ++i) Q[i] = Q[i] - k.E * (t1[i] + t2[i] - 3.0 * WVW[i]);
    m3_mul(WVW, W, t1);
    m3_mul(W, WVW, t2);
    for (int i = 0; i < 9; ++i) Q[i] = Q[i] + k.F * (t1[i] + t2[i]);
}

// Jr(e) = [[Jw, 0], [Q, Jw]]
__host__ __device__ inline void pgo_jr(const double* e, double* Jw, double* Q) {
    const PgoCoef k = pgo_coef(norm3(e));
    so3_poly(e, -k.B, k.C, Jw);
    pgo_q_right(e, k, Q);
}

// Jr^-1(e) = [[Ji, 0], [Q2, Ji]], Q2 = -Ji Q Ji
__host__ __device__ inline void pgo_jr_inv(const double* e, double* Ji, double* Q2) {
    const PgoCoef k = pgo_coef(norm3(e));
    double Q[9], t[9];
    so3_poly(e, 0.5, k.D, Ji);
    pgo_q_right(e, k, Q);
    m3_mul(Ji, Q, t);
    m3_mul(t, Ji, Q2);
    for (int i = 0; i < 9; ++i) Q2[i] = -Q2[i];
}

}  // namespace ndt
