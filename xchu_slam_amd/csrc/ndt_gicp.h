// ndt_gicp.h — device-resident state and control step of the Generalized-ICP operator (gicp.hip, host_gicp.hip).
//
// pclomp::GeneralizedIterativeClosestPoint (gicp_omp_impl.hpp) with the project's own minimiser (GICP):
// k_gicp_pairs is one outer iteration's correspondence step, k_gicp_eval one evaluation of the objective and its
// gradient at the state's trial point.  The last workgroup of either runs the control step below, so a fixed sequence
// of launches needs no host round trip: a launch whose phase is not the state's returns at its first load.
// The control step is host/device code (NDT_HD): tests/native/gicp_control_check.cpp runs the same text with a host
// evaluator.  tests/gicp_restate.py is its definition, statement for statement.
#pragma once
#include "ndt_linalg.h"

namespace ndt {

constexpr int kGicpBlock = 256;                      // threads per workgroup of the three kernels
constexpr int kGicpTeam = 16;                        // lanes per point (k_gicp_cov, k_gicp_pairs)
constexpr int kGicpTeams = kGicpBlock / kGicpTeam;   // points per workgroup step
constexpr int kGicpMaxBlocks = 1024;                 // grid cap of k_gicp_pairs
constexpr int kGicpCovMaxBlocks = 8192;              // grid cap of k_gicp_cov (131 072 points per trip of its loop)
constexpr int kGicpEvalBlocks = 256;                 // grid cap of k_gicp_eval: the tail sums 13 partials per workgroup
constexpr int kGicpSums = 13;                        // f, sum temp[3], sum (guess p) temp^T [9]
constexpr int kGicpMaxHistory = 1024;                // per-iteration records kept
constexpr int kGicpMaxK = 32;                        // largest k_correspondences
// the minimiser's caps (gicp_restate.py: MAX_EVALS, MAX_BRACKET, MAX_SECTION)
constexpr int kGicpMaxEvals = 200;
constexpr int kGicpMaxBracket = 20;
constexpr int kGicpMaxSection = 30;

// ndt_gicp_state of include/ndt_hip.h
enum GicpConv { GICP_NOT_CONVERGED = 0, GICP_ITERATIONS = 1, GICP_DELTA = 2, GICP_NO_CORRESPONDENCES = 3, GICP_SOLVER_FAILED = 4 };
enum GicpMin { GICP_MIN_RUNNING = 0, GICP_MIN_SUCCESS = 1, GICP_MIN_NO_PROGRESS = 2, GICP_MIN_MAX_INNER = 3, GICP_MIN_FAILED = 4 };
enum GicpPhase { GICP_PAIRS = 0, GICP_EVAL = 1, GICP_DONE = 2, GICP_EVAL_ONLY = 3 };

// The minimiser: BFGS (inverse-Hessian form) with Fletcher's bracketing / sectioning line search, one evaluation per
// step (Minimiser of gicp_restate.py)
struct GicpMinimiser {
    int phase;              // 0 initial evaluation, 1 bracketing, 2 sectioning
    int status;             // GicpMin
    int evals, inner, ls_i, max_inner;
    double x[6];            // the trial point
    double x0[6], g0[6], p[6], H[36];
    double f0, g0norm, pnorm, fp0;
    double alpha, alpha_prev, falpha_prev, fpalpha_prev;
    double a, fa, fpa, b, fb, fpb;
};

struct GicpState {
    // ---- constants of this align ----
    double corr2;           // max_corr_dist^2 (a pair is kept when (double)d2 < corr2)
    double rot_eps, trans_eps;
    int max_iter, max_inner;
    float guess[16];        // column-major
    // ---- state ----
    int phase;              // GicpPhase
    int converged, conv_state, iterations;
    int pairs;              // pairs of the last outer iteration
    int pair_count;         // k_gicp_pairs' running count (atomic), cleared by its last workgroup
    int hist_count, total_evals;
    double f_last;
    double Rtg[9];          // top-left corner of transformation_ * guess in f64, column-major (k_gicp_pairs' R)
    float trans[16];        // transformation_
    float prev[16];         // previous_transformation_
    float T_trial[16];      // applyState(guess, x) at the trial point: what k_gicp_eval applies
    float final_tf[16];
    double ev_f, ev_g[6];   // GICP_EVAL_ONLY: the objective at min.x
    GicpMinimiser min;
};

struct GicpRecordDev {
    float T[16];            // transformation_ after the iteration
    double f, delta;
    int pairs, inner, evals, status, conv_state, pad;
};

// ------------------------------------------------------------------------------------------------ the minimiser
NDT_HD double gicp_norm6(const double* v) {
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += v[k] * v[k];
    return sqrt(s);
}
NDT_HD double gicp_dot6(const double* u, const double* v) {
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += u[k] * v[k];
    return s;
}
NDT_HD double gicp_cubic(double c0, double c1, double c2, double c3, double z) { return c0 + z * (c1 + z * (c2 + z * c3)); }

// interp_cubic of gicp_restate.py
NDT_HD double gicp_interp(double a, double fa, double fpa, double b, double fb, double fpb, double xmin, double xmax) {
    const double ba = b - a;
    double zl = (xmin - a) / ba, zh = (xmax - a) / ba;
    if (zl > zh) { const double t = zl; zl = zh; zh = t; }
    const double f0 = fa, fp0 = fpa * ba, f1 = fb, fp1 = fpb * ba;
    const double eta = 3.0 * (f1 - f0) - 2.0 * fp0 - fp1;
    const double xi = fp0 + fp1 - 2.0 * (f1 - f0);
    const double c0 = f0, c1 = fp0, c2 = eta, c3 = xi;
    double zmin = zl, fmin = gicp_cubic(c0, c1, c2, c3, zl);
    double cand[3];
    int nc = 0;
    cand[nc++] = zh;
    const double qa = 3.0 * c3, qb = 2.0 * c2, qc = c1;
    if (qa == 0.0) {
        if (qb != 0.0) cand[nc++] = -qc / qb;
    } else {
        const double disc = qb * qb - 4.0 * qa * qc;
        if (disc > 0.0) {
            const double sq = sqrt(disc);
            const double r0 = (-qb - sq) / (2.0 * qa), r1 = (-qb + sq) / (2.0 * qa);
            cand[nc++] = r0 < r1 ? r0 : r1;
            cand[nc++] = r0 < r1 ? r1 : r0;
        } else if (disc == 0.0) {
            cand[nc++] = -qb / (2.0 * qa);
        }
    }
    for (int k = 0; k < 3; ++k) {
        if (k >= nc) break;
        const double z = cand[k];
        if (k > 0 && !(zl < z && z < zh)) continue;
        const double y = gicp_cubic(c0, c1, c2, c3, z);
        if (y < fmin) { zmin = z; fmin = y; }
    }
    return a + zmin * ba;
}

// every function below returns true when m->x holds a new trial point, false when m->status has left RUNNING
NDT_HD bool gicp_min_finish(GicpMinimiser* m, int status) {
    m->status = status;
    return false;
}
NDT_HD bool gicp_min_trial(GicpMinimiser* m, double alpha) {
    m->alpha = alpha;
    for (int k = 0; k < 6; ++k) m->x[k] = m->x0[k] + alpha * m->p[k];
    return true;
}
NDT_HD bool gicp_min_start_step(GicpMinimiser* m) {
    m->inner += 1;
    if (m->pnorm == 0.0 || m->g0norm == 0.0 || m->fp0 == 0.0) return gicp_min_finish(m, GICP_MIN_NO_PROGRESS);
    // the first trial step: a unit-length move along -g in the first line search, the quasi-Newton step after it
    const double alpha1 = m->inner == 1 ? 1.0 / m->g0norm : 1.0;
    m->alpha_prev = 0.0;
    m->falpha_prev = m->f0;
    m->fpalpha_prev = m->fp0;
    m->ls_i = 0;
    m->phase = 1;
    return gicp_min_trial(m, alpha1);
}
NDT_HD bool gicp_min_section_trial(GicpMinimiser* m) {
    const double delta = m->b - m->a;
    return gicp_min_trial(m, gicp_interp(m->a, m->fa, m->fpa, m->b, m->fb, m->fpb, m->a + 0.05 * delta, m->b - 0.5 * delta));
}
NDT_HD bool gicp_min_go_section(GicpMinimiser* m) {
    m->phase = 2;
    m->ls_i = 0;
    return gicp_min_section_trial(m);
}
NDT_HD void gicp_min_identity(double* H) {
    for (int k = 0; k < 36; ++k) H[k] = (k % 7 == 0) ? 1.0 : 0.0;
}
NDT_HD bool gicp_min_accept(GicpMinimiser* m, double f, const double* g) {
    m->f0 = f;
    double s[6], y[6];
    for (int k = 0; k < 6; ++k) { s[k] = m->x[k] - m->x0[k]; y[k] = g[k] - m->g0[k]; }
    const double sy = gicp_dot6(s, y);
    if (sy > 0.0) {  // the curvature condition; otherwise H is kept
        double Hy[6];
        for (int i = 0; i < 6; ++i) Hy[i] = gicp_dot6(m->H + 6 * i, y);
        const double c1 = (sy + gicp_dot6(y, Hy)) / (sy * sy);
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j)
                m->H[6 * i + j] = (m->H[6 * i + j] + c1 * s[i] * s[j]) - (Hy[i] * s[j] + s[i] * Hy[j]) / sy;
    }
    double p[6];
    for (int i = 0; i < 6; ++i) p[i] = -gicp_dot6(m->H + 6 * i, g);
    double fp0 = gicp_dot6(p, g);
    if (!(fp0 < 0.0)) {  // not a descent direction: restart from steepest descent
        gicp_min_identity(m->H);
        for (int i = 0; i < 6; ++i) p[i] = -g[i];
        fp0 = gicp_dot6(p, g);
    }
    for (int k = 0; k < 6; ++k) { m->g0[k] = g[k]; m->x0[k] = m->x[k]; m->p[k] = p[k]; }
    m->g0norm = gicp_norm6(g);
    m->pnorm = gicp_norm6(p);
    m->fp0 = fp0;
    if (m->g0norm < 1e-2) return gicp_min_finish(m, GICP_MIN_SUCCESS);
    if (m->inner >= m->max_inner) return gicp_min_finish(m, GICP_MIN_MAX_INNER);
    return gicp_min_start_step(m);
}
NDT_HD bool gicp_min_bracket(GicpMinimiser* m, double fal, double fpal, const double* g) {
    const double al = m->alpha;
    m->ls_i += 1;
    if (fal > m->f0 + al * 0.01 * m->fp0 || fal >= m->falpha_prev) {
        m->a = m->alpha_prev; m->fa = m->falpha_prev; m->fpa = m->fpalpha_prev;
        m->b = al; m->fb = fal; m->fpb = fpal;
        return gicp_min_go_section(m);
    }
    if (fabs(fpal) <= -0.01 * m->fp0) return gicp_min_accept(m, fal, g);
    if (fpal >= 0.0) {
        m->a = al; m->fa = fal; m->fpa = fpal;
        m->b = m->alpha_prev; m->fb = m->falpha_prev; m->fpb = m->fpalpha_prev;
        return gicp_min_go_section(m);
    }
    if (m->ls_i >= kGicpMaxBracket) return gicp_min_finish(m, GICP_MIN_FAILED);
    const double delta = al - m->alpha_prev;
    const double nxt = gicp_interp(m->alpha_prev, m->falpha_prev, m->fpalpha_prev, al, fal, fpal, al + delta, al + 9.0 * delta);
    m->alpha_prev = al; m->falpha_prev = fal; m->fpalpha_prev = fpal;
    return gicp_min_trial(m, nxt);
}
NDT_HD bool gicp_min_section(GicpMinimiser* m, double fal, double fpal, const double* g) {
    const double al = m->alpha;
    m->ls_i += 1;
    if ((m->a - al) * m->fpa <= DBL_EPSILON) return gicp_min_finish(m, GICP_MIN_NO_PROGRESS);  // round-off: the result stays x0
    if (fal > m->f0 + 0.01 * al * m->fp0 || fal >= m->fa) {
        m->b = al; m->fb = fal; m->fpb = fpal;
    } else {
        if (fabs(fpal) <= -0.01 * m->fp0) return gicp_min_accept(m, fal, g);
        if (((m->b - m->a) >= 0.0 && fpal >= 0.0) || ((m->b - m->a) <= 0.0 && fpal <= 0.0)) {
            m->b = m->a; m->fb = m->fa; m->fpb = m->fpa;
        }
        m->a = al; m->fa = fal; m->fpa = fpal;
    }
    if (m->ls_i >= kGicpMaxSection) return gicp_min_accept(m, fal, g);
    return gicp_min_section_trial(m);
}
NDT_HD void gicp_min_begin(GicpMinimiser* m, const double* x, int max_inner) {
    for (int k = 0; k < 6; ++k) m->x[k] = x[k];
    m->phase = 0;
    m->evals = 0;
    m->inner = 0;
    m->max_inner = max_inner;
    m->status = GICP_MIN_RUNNING;
}
NDT_HD bool gicp_min_feed(GicpMinimiser* m, double f, const double* g) {
    m->evals += 1;
    bool more;
    if (m->phase == 0) {
        for (int k = 0; k < 6; ++k) { m->x0[k] = m->x[k]; m->g0[k] = g[k]; m->p[k] = -g[k]; }
        m->f0 = f;
        m->g0norm = gicp_norm6(g);
        gicp_min_identity(m->H);
        m->pnorm = gicp_norm6(m->p);
        m->fp0 = gicp_dot6(m->p, g);
        more = gicp_min_start_step(m);
    } else {
        const double fp = gicp_dot6(g, m->p);
        more = m->phase == 1 ? gicp_min_bracket(m, f, fp, g) : gicp_min_section(m, f, fp, g);
    }
    if (more && m->evals >= kGicpMaxEvals) return gicp_min_finish(m, GICP_MIN_FAILED);
    return more;
}

// ------------------------------------------------------------------------------------------------ applyState
// AngleAxisf(x[5], Z) * AngleAxisf(x[4], Y) * AngleAxisf(x[3], X) as Eigen 3.3 evaluates it (a product of f32
// quaternions converted to a matrix), column-major R (rotation_of_state of gicp_restate.py)
NDT_HD void gicp_rotation(const double* x, float* R) {
    const float ax = (float)x[3], ay = (float)x[4], az = (float)x[5];
    const float q0[4] = {cosf_dr(0.5f * az), 0.f, 0.f, sinf_dr(0.5f * az)};  // w, x, y, z
    const float q1[4] = {cosf_dr(0.5f * ay), 0.f, sinf_dr(0.5f * ay), 0.f};
    const float q2[4] = {cosf_dr(0.5f * ax), sinf_dr(0.5f * ax), 0.f, 0.f};
    float a[4], q[4];
    a[0] = q0[0] * q1[0] - q0[1] * q1[1] - q0[2] * q1[2] - q0[3] * q1[3];
    a[1] = q0[0] * q1[1] + q0[1] * q1[0] + q0[2] * q1[3] - q0[3] * q1[2];
    a[2] = q0[0] * q1[2] + q0[2] * q1[0] + q0[3] * q1[1] - q0[1] * q1[3];
    a[3] = q0[0] * q1[3] + q0[3] * q1[0] + q0[1] * q1[2] - q0[2] * q1[1];
    q[0] = a[0] * q2[0] - a[1] * q2[1] - a[2] * q2[2] - a[3] * q2[3];
    q[1] = a[0] * q2[1] + a[1] * q2[0] + a[2] * q2[3] - a[3] * q2[2];
    q[2] = a[0] * q2[2] + a[2] * q2[0] + a[3] * q2[1] - a[1] * q2[3];
    q[3] = a[0] * q2[3] + a[3] * q2[0] + a[1] * q2[2] - a[2] * q2[1];
    const float w = q[0], qx = q[1], qy = q[2], qz = q[3];
    const float tx = 2.f * qx, ty = 2.f * qy, tz = 2.f * qz;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const float tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0] = 1.f - (tyy + tzz); R[3] = txy - twz; R[6] = txz + twy;
    R[1] = txy + twz; R[4] = 1.f - (txx + tzz); R[7] = tyz - twx;
    R[2] = txz - twy; R[5] = tyz + twx; R[8] = 1.f - (txx + tyy);
}

// applyState (:517-527) on a column-major 4x4: out.R = R(x) * base.R, out.t = base.t + (float)x[0:3]
NDT_HD void gicp_apply_state(const float* base, const double* x, float* out) {
    float R[9];
    gicp_rotation(x, R);
    for (int k = 0; k < 16; ++k) out[k] = base[k];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            out[i + 4 * j] = (R[i] * base[4 * j] + R[i + 3] * base[1 + 4 * j]) + R[i + 6] * base[2 + 4 * j];
    for (int i = 0; i < 3; ++i) out[12 + i] = base[12 + i] + (float)x[i];
}

// computeRDerivative (:135-186): g[3..5] from Rm (row-major Rm[3 * i + j] = 2/m sum (guess p)_i temp_j)
NDT_HD void gicp_r_derivative(const double* x, const double* Rm, double* g) {
    const double phi = x[3], theta = x[4], psi = x[5];
    const double cphi = cos(phi), sphi = sin(phi), cth = cos(theta), sth = sin(theta), cpsi = cos(psi), spsi = sin(psi);
    // row-major d[3 * row + col]
    const double dphi[9] = {0.0, sphi * spsi + cphi * cpsi * sth, cphi * spsi - cpsi * sphi * sth,
                            0.0, -cpsi * sphi + cphi * spsi * sth, -cphi * cpsi - sphi * spsi * sth,
                            0.0, cphi * cth, -cth * sphi};
    const double dth[9] = {-cpsi * sth, cpsi * cth * sphi, cphi * cpsi * cth,
                           -spsi * sth, cth * sphi * spsi, cphi * cth * spsi,
                           -cth, -sphi * sth, -cphi * sth};
    const double dpsi[9] = {-cth * spsi, -cphi * cpsi - sphi * spsi * sth, cpsi * sphi - cphi * spsi * sth,
                            cpsi * cth, -cphi * spsi + cpsi * sphi * sth, sphi * spsi + cphi * cpsi * sth,
                            0.0, 0.0, 0.0};
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {  // matricesInnerProd: r += mat1(j, i) * mat2(i, j)
            r0 += dphi[3 * j + i] * Rm[3 * i + j];
            r1 += dth[3 * j + i] * Rm[3 * i + j];
            r2 += dpsi[3 * j + i] * Rm[3 * i + j];
        }
    g[3] = r0; g[4] = r1; g[5] = r2;
}

// f and g at x from the 13 sums over m pairs (S[0] sum res.temp, S[1..3] sum temp, S[4 + 3 i + j] sum (guess p)_i temp_j)
NDT_HD void gicp_fg_of_sums(const double* S, int m, const double* x, double* f, double* g) {
    *f = S[0] / (double)m;
    const double s2 = 2.0 / (double)m;
    for (int k = 0; k < 3; ++k) g[k] = S[1 + k] * s2;
    double Rm[9];
    for (int k = 0; k < 9; ++k) Rm[k] = S[4 + k] * s2;
    gicp_r_derivative(x, Rm, g);
}

// ------------------------------------------------------------------------------------------------ the outer loop
NDT_HD void gicp_identity16(float* T) {
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
}

// transform_R (:422-428): the corner of transformation_ * guess in f64 (products of the f32 entries, k = 0..3 from zero)
NDT_HD void gicp_set_rtg(GicpState* st) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += (double)st->trans[i + 4 * k] * (double)st->guess[k + 4 * j];
            st->Rtg[i + 3 * j] = s;
        }
}

// :507-510: final.R = prev.R * guess.R (f32), final.t = prev.t + guess.t
NDT_HD void gicp_set_final(GicpState* st) {
    gicp_identity16(st->final_tf);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            st->final_tf[i + 4 * j] = (st->prev[i] * st->guess[4 * j] + st->prev[i + 4] * st->guess[1 + 4 * j]) + st->prev[i + 8] * st->guess[2 + 4 * j];
        st->final_tf[12 + i] = st->prev[12 + i] + st->guess[12 + i];
    }
}

NDT_HD void gicp_record(GicpState* st, GicpRecordDev* hist, double f, double delta, int inner, int evals, int status, int conv) {
    const int hc = st->hist_count;
    if (hc < kGicpMaxHistory) {
        GicpRecordDev* r = hist + hc;
        for (int k = 0; k < 16; ++k) r->T[k] = st->trans[k];
        r->f = f;
        r->delta = delta;
        r->pairs = st->pairs;
        r->inner = inner;
        r->evals = evals;
        r->status = status;
        r->conv_state = conv;
        r->pad = 0;
    }
    st->hist_count = hc + 1;
}

NDT_HD void gicp_end_unconverged(GicpState* st, GicpRecordDev* hist, int conv, double f, int inner, int evals, int status) {
    st->conv_state = conv;
    st->converged = 0;
    gicp_record(st, hist, f, 0.0, inner, evals, status, conv);
    gicp_set_final(st);  // from the transformation before the attempt
    st->phase = GICP_DONE;
}

// After k_gicp_pairs: the pair-count test and the start of the inner solve (the initial x, :203-209)
NDT_HD void gicp_after_pairs(GicpState* st, GicpRecordDev* hist, int pairs) {
    st->pairs = pairs;
    for (int k = 0; k < 16; ++k) st->prev[k] = st->trans[k];
    if (pairs < 4) {
        gicp_end_unconverged(st, hist, GICP_NO_CORRESPONDENCES, 0.0, 0, 0, GICP_MIN_RUNNING);
        return;
    }
    const float* T = st->trans;
    double x[6] = {(double)T[12], (double)T[13], (double)T[14], atan2((double)T[6], (double)T[10]), asin(-(double)T[2]),
                   atan2((double)T[1], (double)T[0])};
    gicp_min_begin(&st->min, x, st->max_inner);
    gicp_apply_state(st->guess, st->min.x, st->T_trial);
    st->phase = GICP_EVAL;
}

// After k_gicp_eval: one step of the minimiser; at the end of a solve the delta test and the switch back to the pairs phase
NDT_HD void gicp_after_eval(GicpState* st, GicpRecordDev* hist, const double* S) {
    double f, g[6];
    gicp_fg_of_sums(S, st->pairs, st->min.x, &f, g);
    if (st->phase == GICP_EVAL_ONLY) {
        st->ev_f = f;
        for (int k = 0; k < 6; ++k) st->ev_g[k] = g[k];
        st->phase = GICP_DONE;
        return;
    }
    st->total_evals += 1;
    GicpMinimiser* m = &st->min;
    if (gicp_min_feed(m, f, g)) {
        gicp_apply_state(st->guess, m->x, st->T_trial);
        return;
    }
    st->f_last = m->f0;
    if (m->status == GICP_MIN_FAILED) {
        gicp_end_unconverged(st, hist, GICP_SOLVER_FAILED, m->f0, m->inner, m->evals, m->status);
        return;
    }
    float id[16];
    gicp_identity16(id);
    gicp_apply_state(id, m->x0, st->trans);
    double delta = 0.0;
    for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 4; ++l) {
            const double ratio = (k < 3 && l < 3) ? 1.0 / st->rot_eps : 1.0 / st->trans_eps;
            const double c = ratio * fabs((double)(st->prev[k + 4 * l] - st->trans[k + 4 * l]));  // an f32 difference
            if (c > delta) delta = c;
        }
    const int it = ++st->iterations;
    int conv = GICP_NOT_CONVERGED;
    if (it >= st->max_iter) conv = GICP_ITERATIONS;
    else if (delta < 1.0) conv = GICP_DELTA;
    st->conv_state = conv;
    gicp_record(st, hist, m->f0, delta, m->inner, m->evals, m->status, conv);
    if (conv != GICP_NOT_CONVERGED) {
        st->converged = 1;
        for (int k = 0; k < 16; ++k) st->prev[k] = st->trans[k];
        gicp_set_final(st);
        st->phase = GICP_DONE;
    } else {
        gicp_set_rtg(st);
        st->phase = GICP_PAIRS;
    }
}

}  // namespace ndt
