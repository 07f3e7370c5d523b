"""numpy restatement of the Generalized-ICP semantics the device implements (GICP section: pclomp's
GeneralizedIterativeClosestPoint, gicp_omp_impl.hpp, with the project's own BFGS minimiser in place of PCL's bfgs.h,
which is not part of the reference tree).  PCL is not available, and the reference's OpenMP sums have no fixed order:
this restatement is the specification's executable form (parity with PCL unpinned).

Operation order, as the device has it:
  * f32 transforms are ((T0 x + T4 y) + T8 z) + T12 per row (icp_restate.transform_f32);
  * 3-term f64 products are (a0 b0 + a1 b1) + a2 b2;
  * every f64 sum over neighbours or pairs runs sequentially in the stated order (np.cumsum), the device's pair sums
    through a fixed tree instead: the only difference, measured by `pair_order`;
  * sinf / cosf are the correctly rounded f32 values (sinf_dr / cosf_dr of ndt_libm.h);
  * the covariance SVD is numpy's (the device runs svd_jacobi): the rebuilt matrix agrees wherever the two smallest
    singular values are apart.
"""
import math

import numpy as np
from scipy.spatial import cKDTree

from icp_restate import F32, WORKERS, Target, correspondences, l2_simple_f32, transform_f32

NOT_CONVERGED, ITERATIONS, DELTA, NO_CORRESPONDENCES, SOLVER_FAILED = range(5)
STATE_NAMES = ("NOT_CONVERGED", "ITERATIONS", "DELTA", "NO_CORRESPONDENCES", "SOLVER_FAILED")
# minimiser status of one inner solve
MIN_RUNNING, MIN_SUCCESS, MIN_NO_PROGRESS, MIN_MAX_INNER, MIN_FAILED = range(5)
MIN_NAMES = ("RUNNING", "SUCCESS", "NO_PROGRESS", "MAX_INNER", "FAILED")

DEFAULTS = dict(max_corr_dist=5.0, max_iter=200, trans_eps=5e-4, rot_eps=2e-3, k_correspondences=20, gicp_epsilon=1e-3,
                max_inner_iter=20)
RHO, SIGMA, TAU1, TAU2, TAU3 = 0.01, 0.01, 9.0, 0.05, 0.5
GRAD_TOL = 1e-2
MAX_EVALS = 200      # evaluations per solve: past it the solve is FAILED
MAX_BRACKET = 20     # bracketing trials per line search: past it the solve is FAILED
MAX_SECTION = 30     # sectioning trials per line search: past it the last trial is taken
DBL_EPS = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------------ covariances
def knn_order(pts, k, extra=8):
    """The k nearest neighbours of every point within its own cloud, the point included, ascending (d2 as f32
    L2_Simple, original index).  The tree proposes k + extra candidates; the f32 value and the index decide.  Returns
    (index (n, k), d2 (n, k), the next candidate's d2 or inf)."""
    pts = np.ascontiguousarray(np.asarray(pts, F32)[:, :3])
    n = len(pts)
    kk = min(n, k + extra)
    _, ii = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=kk, workers=WORKERS)
    ii = ii.reshape(n, kk)
    d2 = l2_simple_f32(pts[ii], pts[:, None, :])
    order = np.lexsort((ii, d2), axis=1)  # by d2, then by index
    ii = np.take_along_axis(ii, order, 1)
    d2 = np.take_along_axis(d2, order, 1)
    nxt = d2[:, k] if kk > k else np.full(n, np.inf, F32)
    return ii[:, :k], d2[:, :k], nxt


def knn_bruteforce(pts, k):
    """knn_order over every pair (exact under any number of ties; small clouds only)."""
    pts = np.ascontiguousarray(np.asarray(pts, F32)[:, :3])
    d2 = l2_simple_f32(pts[None, :, :], pts[:, None, :])
    ii = np.broadcast_to(np.arange(len(pts)), d2.shape)
    order = np.lexsort((ii, d2), axis=1)[:, :k]
    return order, np.take_along_axis(d2, order, 1)


def covariances(pts, k=20, gicp_epsilon=1e-3, nn=None):
    """computeCovariances (:59-131).  Returns (regularised (n, 3, 3), raw (n, 3, 3), singular values (n, 3)).
    nn: the neighbour indices (n, k) in summation order (default knn_order's)."""
    pts = np.ascontiguousarray(np.asarray(pts, F32)[:, :3])
    n = len(pts)
    if n < k:
        raise ValueError("fewer points than k_correspondences")
    if nn is None:
        nn = knn_order(pts, k)[0]
    mean = np.zeros((n, 3))
    cov = np.zeros((n, 3, 3))
    for j in range(k):  # the sums run in neighbour order; each product is an f32 product added to an f64 sum
        p = pts[nn[:, j]]
        mean += p.astype(np.float64)
        for a in range(3):
            for b in range(a + 1):
                cov[:, a, b] += (p[:, a] * p[:, b]).astype(np.float64)
    mean /= float(k)
    for a in range(3):
        for b in range(a + 1):
            cov[:, a, b] /= float(k)
            cov[:, a, b] -= mean[:, a] * mean[:, b]
            cov[:, b, a] = cov[:, a, b]
    U, s, _ = np.linalg.svd(cov)
    out = np.zeros((n, 3, 3))
    for c, v in enumerate((1.0, 1.0, gicp_epsilon)):
        out += v * U[:, :, c, None] * U[:, None, :, c]
    return out, cov, s


# ------------------------------------------------------------------------------------------------ applyState
def sinf_dr(a):
    return F32(math.sin(float(F32(a))))


def cosf_dr(a):
    return F32(math.cos(float(F32(a))))


def _quat_mul(a, b):
    """Eigen's quaternion product (w, x, y, z), each component left to right."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx)


def rotation_of_state(x, dtype=F32):
    """AngleAxis(x[5], Z) * AngleAxis(x[4], Y) * AngleAxis(x[3], X) as Eigen 3.3 evaluates it: a product of quaternions
    (half-angle sin / cos) converted to a matrix.  dtype f32 is the literal route, f64 the exact one."""
    f = dtype
    if dtype is F32:
        sn, cs = sinf_dr, cosf_dr
        half = F32(0.5)
        ang = [F32(x[3]), F32(x[4]), F32(x[5])]
    else:
        sn, cs = math.sin, math.cos
        half = 0.5
        ang = [float(x[3]), float(x[4]), float(x[5])]
    zero = f(0)
    qx = (f(cs(half * ang[0])), f(sn(half * ang[0])), zero, zero)
    qy = (f(cs(half * ang[1])), zero, f(sn(half * ang[1])), zero)
    qz = (f(cs(half * ang[2])), zero, zero, f(sn(half * ang[2])))
    w, qx_, qy_, qz_ = _quat_mul(_quat_mul(qz, qy), qx)
    two, one = f(2), f(1)
    tx, ty, tz = two * qx_, two * qy_, two * qz_
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * qx_, ty * qx_, tz * qx_
    tyy, tyz, tzz = ty * qy_, tz * qy_, tz * qz_
    R = np.empty((3, 3), dtype)
    R[0] = [one - (tyy + tzz), txy - twz, txz + twy]
    R[1] = [txy + twz, one - (txx + tzz), tyz - twx]
    R[2] = [txz - twy, tyz + twx, one - (txx + tyy)]
    return R


def apply_state(base, x, dtype=F32):
    """applyState (:517-527): t.R = R(x) * t.R, t.t += x[0:3], in dtype."""
    base = np.asarray(base, dtype)
    R = rotation_of_state(x, dtype)
    T = base.copy()
    B = base[:3, :3]
    for i in range(3):
        for j in range(3):
            T[i, j] = (R[i, 0] * B[0, j] + R[i, 1] * B[1, j]) + R[i, 2] * B[2, j]
    for i in range(3):
        T[i, 3] = base[i, 3] + dtype(x[i])
    return T


def state_of_transform(T):
    """The initial x of a solve (:203-209): f64 atan2 / asin of the f32 entries."""
    T = np.asarray(T, F32)
    return np.array([float(T[0, 3]), float(T[1, 3]), float(T[2, 3]), math.atan2(float(T[2, 1]), float(T[2, 2])),
                     math.asin(-float(T[2, 0])), math.atan2(float(T[1, 0]), float(T[0, 0]))])


def r_derivative(x, Rm):
    """computeRDerivative (:135-186) with f64 sin and cos: g[3:6] from Rm = 2/m sum (guess p) temp^T."""
    phi, theta, psi = float(x[3]), float(x[4]), float(x[5])
    cphi, sphi = math.cos(phi), math.sin(phi)
    cth, sth = math.cos(theta), math.sin(theta)
    cpsi, spsi = math.cos(psi), math.sin(psi)
    dphi = np.array([[0.0, sphi * spsi + cphi * cpsi * sth, cphi * spsi - cpsi * sphi * sth],
                     [0.0, -cpsi * sphi + cphi * spsi * sth, -cphi * cpsi - sphi * spsi * sth],
                     [0.0, cphi * cth, -cth * sphi]])
    dth = np.array([[-cpsi * sth, cpsi * cth * sphi, cphi * cpsi * cth],
                    [-spsi * sth, cth * sphi * spsi, cphi * cth * spsi],
                    [-cth, -sphi * sth, -cphi * sth]])
    dpsi = np.array([[-cth * spsi, -cphi * cpsi - sphi * spsi * sth, cpsi * sphi - cphi * spsi * sth],
                     [cpsi * cth, -cphi * spsi + cpsi * sphi * sth, sphi * spsi + cphi * cpsi * sth],
                     [0.0, 0.0, 0.0]])
    out = []
    for d in (dphi, dth, dpsi):  # matricesInnerProd: r += mat1(j, i) * mat2(i, j), i outer, j inner
        r = 0.0
        for i in range(3):
            for j in range(3):
                r += d[j, i] * Rm[i, j]
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ pairs, objective
def mat4_mul_f64(A, B):
    """transform_R (:422-426): f64 products of the f32 entries, summed k = 0..3 from zero."""
    A = np.asarray(A, F32).astype(np.float64)
    B = np.asarray(B, F32).astype(np.float64)
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            for k in range(4):
                C[i, j] += A[i, k] * B[k, j]
    return C


def _mul3(A, B):
    """batched 3x3 product, (a0 b0 + a1 b1) + a2 b2"""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def inverse3(m):
    """Eigen's 3x3 inverse by cofactors (inverse3 of ndt_linalg.h), batched over the leading axis."""
    def cof(i, j):
        return (m[:, (i + 1) % 3, (j + 1) % 3] * m[:, (i + 2) % 3, (j + 2) % 3]
                - m[:, (i + 1) % 3, (j + 2) % 3] * m[:, (i + 2) % 3, (j + 1) % 3])
    c0, c1, c2 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = c0 * m[:, 0, 0] + c1 * m[:, 1, 0] + c2 * m[:, 2, 0]
    inv = 1.0 / det
    r = np.empty_like(m)
    r[:, 0, 0], r[:, 0, 1], r[:, 0, 2] = c0 * inv, c1 * inv, c2 * inv
    for i in (1, 2):
        for j in range(3):
            r[:, i, j] = cof(j, i) * inv
    return r


class Pairs:
    """The correspondences of one outer iteration and what the objective reads of them."""

    def __init__(self, source, tgt: Target, guess, trans, cov_src, cov_tgt, max_corr_dist, exact=False):
        src = np.ascontiguousarray(np.asarray(source, F32)[:, :3])
        self.gp_all = transform_f32(guess, src)             # guess * p
        X = transform_f32(trans, self.gp_all)               # transformation_ * (guess * p)
        idx, d2, ties = correspondences(X, tgt, exact=exact)
        keep = (idx >= 0) & (d2.astype(np.float64) < float(max_corr_dist) * float(max_corr_dist))  # strict
        self.index = np.where(keep, idx, -1)
        self.d2, self.ties = d2, ties
        self.sel = np.flatnonzero(keep)
        self.m = len(self.sel)
        R = mat4_mul_f64(trans, guess)[:3, :3]
        j = idx[self.sel]
        Rb = np.broadcast_to(R, (self.m, 3, 3))
        temp = _mul3(_mul3(Rb, cov_src[self.sel]), np.broadcast_to(R.T, (self.m, 3, 3))) + cov_tgt[j]
        self.M = inverse3(temp)
        self.p = src[self.sel]
        self.q = tgt.pts[j]
        self.gp = self.gp_all[self.sel]
        self.guess = np.asarray(guess, F32)


def _seqsum(v, order):
    v = v if order is None else v[order]
    return np.cumsum(v, axis=0)[-1]


def objective(pairs: Pairs, x, transform_dtype=F32, pair_order=None):
    """fdf (:344-377) at x.  Returns (f, g[6]).  pair_order: None = index order, or a permutation of range(m)."""
    m = pairs.m
    T = apply_state(pairs.guess, x, transform_dtype)
    if transform_dtype is F32:
        pp = transform_f32(T, pairs.p)
        res = (pp - pairs.q).astype(np.float64)            # an f32 subtraction widened
    else:
        P = pairs.p.astype(np.float64)
        pp = np.stack([((T[a, 0] * P[:, 0] + T[a, 1] * P[:, 1]) + T[a, 2] * P[:, 2]) + T[a, 3] for a in range(3)], 1)
        res = pp - pairs.q.astype(np.float64)
    M = pairs.M
    temp = np.stack([(M[:, a, 0] * res[:, 0] + M[:, a, 1] * res[:, 1]) + M[:, a, 2] * res[:, 2] for a in range(3)], 1)
    fterm = (res[:, 0] * temp[:, 0] + res[:, 1] * temp[:, 1]) + res[:, 2] * temp[:, 2]
    gp = pairs.gp.astype(np.float64)
    f = float(_seqsum(fterm, pair_order)) / m
    g = np.zeros(6)
    g[:3] = _seqsum(temp, pair_order) * (2.0 / m)
    Rm = _seqsum((gp[:, :, None] * temp[:, None, :]).reshape(m, 9), pair_order).reshape(3, 3) * (2.0 / m)
    g[3:] = r_derivative(x, Rm)
    return f, g


# ------------------------------------------------------------------------------------------------ the minimiser
def _norm(v):
    s = 0.0
    for a in v:
        s += a * a
    return math.sqrt(s)


def _dot(u, v):
    s = 0.0
    for a, b in zip(u, v):
        s += a * b
    return s


def _cubic(c0, c1, c2, c3, z):
    return c0 + z * (c1 + z * (c2 + z * c3))


def interp_cubic(a, fa, fpa, b, fb, fpb, xmin, xmax):
    """The minimiser of the Hermite cubic through (a, fa, fpa), (b, fb, fpb) over [xmin, xmax] (normalised to
    z = (alpha - a) / (b - a)): the lower end, the upper end, then the interior stationary points in ascending root
    order, each taking over when strictly lower."""
    ba = b - a
    zl, zh = (xmin - a) / ba, (xmax - a) / ba
    if zl > zh:
        zl, zh = zh, zl
    f0, fp0, f1, fp1 = fa, fpa * ba, fb, fpb * ba
    eta = 3.0 * (f1 - f0) - 2.0 * fp0 - fp1
    xi = fp0 + fp1 - 2.0 * (f1 - f0)
    c0, c1, c2, c3 = f0, fp0, eta, xi
    zmin, fmin = zl, _cubic(c0, c1, c2, c3, zl)
    cand = [zh]
    qa, qb, qc = 3.0 * c3, 2.0 * c2, c1  # the derivative's quadratic
    if qa == 0.0:
        if qb != 0.0:
            cand.append(-qc / qb)
    else:
        disc = qb * qb - 4.0 * qa * qc
        if disc > 0.0:
            sq = math.sqrt(disc)
            r0, r1 = (-qb - sq) / (2.0 * qa), (-qb + sq) / (2.0 * qa)
            cand += [min(r0, r1), max(r0, r1)]
        elif disc == 0.0:
            cand.append(-qb / (2.0 * qa))
    for k, z in enumerate(cand):
        if k > 0 and not (zl < z < zh):
            continue
        y = _cubic(c0, c1, c2, c3, z)
        if y < fmin:
            zmin, fmin = z, y
    return a + zmin * ba


class Minimiser:
    """BFGS (inverse-Hessian form, H0 = I) with Fletcher's bracketing / sectioning line search, driven one evaluation at a time:
    begin(x) gives the first trial point, feed(f, g) takes the objective there and gives the next trial point, or None
    once `status` has left MIN_RUNNING (the result is then x0, f0)."""

    def __init__(self, max_inner=20):
        self.max_inner = max_inner

    def begin(self, x):
        self.x = np.array(x, np.float64)
        self.phase = 0  # 0 initial evaluation, 1 bracketing, 2 sectioning
        self.evals = self.inner = 0
        self.status = MIN_RUNNING
        return self.x

    def feed(self, f, g):
        self.evals += 1
        g = [float(v) for v in g]
        if self.phase == 0:
            self.x0, self.f0, self.g0 = self.x.copy(), f, list(g)
            self.g0norm = _norm(g)
            self.H = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
            self.p = [-v for v in g]
            self.pnorm = _norm(self.p)
            self.fp0 = _dot(self.p, g)
            nxt = self._start_step()
        else:
            fp = _dot(g, self.p)
            nxt = self._bracket(f, fp, g) if self.phase == 1 else self._section(f, fp, g)
        if nxt is not None and self.evals >= MAX_EVALS:
            return self._finish(MIN_FAILED)
        return nxt

    def _finish(self, status):
        self.status = status
        return None

    def _trial(self, alpha):
        self.alpha = alpha
        self.x = np.array([self.x0[k] + alpha * self.p[k] for k in range(6)])
        return self.x

    def _start_step(self):
        self.inner += 1
        if self.pnorm == 0.0 or self.g0norm == 0.0 or self.fp0 == 0.0:
            return self._finish(MIN_NO_PROGRESS)
        # the first trial step: a unit-length move along -g in the first line search, the quasi-Newton step after it
        alpha1 = 1.0 / self.g0norm if self.inner == 1 else 1.0
        self.alpha_prev, self.falpha_prev, self.fpalpha_prev = 0.0, self.f0, self.fp0
        self.ls_i = 0
        self.phase = 1
        return self._trial(alpha1)

    def _bracket(self, fal, fpal, g):
        al = self.alpha
        self.ls_i += 1
        if fal > self.f0 + al * RHO * self.fp0 or fal >= self.falpha_prev:
            self.a, self.fa, self.fpa = self.alpha_prev, self.falpha_prev, self.fpalpha_prev
            self.b, self.fb, self.fpb = al, fal, fpal
            return self._go_section()
        if abs(fpal) <= -SIGMA * self.fp0:
            return self._accept(fal, g)
        if fpal >= 0.0:
            self.a, self.fa, self.fpa = al, fal, fpal
            self.b, self.fb, self.fpb = self.alpha_prev, self.falpha_prev, self.fpalpha_prev
            return self._go_section()
        if self.ls_i >= MAX_BRACKET:
            return self._finish(MIN_FAILED)
        delta = al - self.alpha_prev
        nxt = interp_cubic(self.alpha_prev, self.falpha_prev, self.fpalpha_prev, al, fal, fpal, al + delta, al + TAU1 * delta)
        self.alpha_prev, self.falpha_prev, self.fpalpha_prev = al, fal, fpal
        return self._trial(nxt)

    def _go_section(self):
        self.phase = 2
        self.ls_i = 0
        return self._section_trial()

    def _section_trial(self):
        delta = self.b - self.a
        return self._trial(interp_cubic(self.a, self.fa, self.fpa, self.b, self.fb, self.fpb, self.a + TAU2 * delta,
                                        self.b - TAU3 * delta))

    def _section(self, fal, fpal, g):
        al = self.alpha
        self.ls_i += 1
        if (self.a - al) * self.fpa <= DBL_EPS:
            return self._finish(MIN_NO_PROGRESS)  # round-off: the result stays x0
        if fal > self.f0 + RHO * al * self.fp0 or fal >= self.fa:
            self.b, self.fb, self.fpb = al, fal, fpal
        else:
            if abs(fpal) <= -SIGMA * self.fp0:
                return self._accept(fal, g)
            if ((self.b - self.a) >= 0.0 and fpal >= 0.0) or ((self.b - self.a) <= 0.0 and fpal <= 0.0):
                self.b, self.fb, self.fpb = self.a, self.fa, self.fpa
            self.a, self.fa, self.fpa = al, fal, fpal
        if self.ls_i >= MAX_SECTION:
            return self._accept(fal, g)
        return self._section_trial()

    def _accept(self, f, g):
        x = self.x
        self.f0 = f
        s = [x[k] - self.x0[k] for k in range(6)]
        y = [g[k] - self.g0[k] for k in range(6)]
        sy = _dot(s, y)
        H = self.H
        if sy > 0.0:  # the curvature condition; otherwise H is kept
            Hy = [_dot(H[i], y) for i in range(6)]
            c1 = (sy + _dot(y, Hy)) / (sy * sy)
            for i in range(6):
                for j in range(6):
                    H[i][j] = (H[i][j] + c1 * s[i] * s[j]) - (Hy[i] * s[j] + s[i] * Hy[j]) / sy
        p = [-_dot(H[i], g) for i in range(6)]
        fp0 = _dot(p, g)
        if not fp0 < 0.0:  # not a descent direction: restart from steepest descent
            self.H = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
            p = [-v for v in g]
            fp0 = _dot(p, g)
        self.g0, self.x0 = list(g), x.copy()
        self.g0norm = _norm(g)
        self.p, self.pnorm, self.fp0 = p, _norm(p), fp0
        if self.g0norm < GRAD_TOL:
            return self._finish(MIN_SUCCESS)
        if self.inner >= self.max_inner:
            return self._finish(MIN_MAX_INNER)
        return self._start_step()


def solve(pairs: Pairs, x_init, max_inner=20, transform_dtype=F32, pair_order=None):
    """One inner solve.  Returns (x, f, status, inner iterations, the trial points in evaluation order)."""
    mn = Minimiser(max_inner)
    x = mn.begin(x_init)
    trials = []
    while x is not None:
        trials.append(x.copy())
        f, g = objective(pairs, x, transform_dtype, pair_order)
        x = mn.feed(f, g)
    return mn.x0.copy(), mn.f0, mn.status, mn.inner, trials


# ------------------------------------------------------------------------------------------------ the outer loop
def final_of(prev, guess):
    """:507-510: R = prev.R * guess.R (f32), t = prev.t + guess.t."""
    prev = np.asarray(prev, F32)
    guess = np.asarray(guess, F32)
    out = np.eye(4, dtype=F32)
    for i in range(3):
        for j in range(3):
            out[i, j] = (prev[i, 0] * guess[0, j] + prev[i, 1] * guess[1, j]) + prev[i, 2] * guess[2, j]
        out[i, 3] = prev[i, 3] + guess[i, 3]
    return out


def gicp(source, target, guess=None, tgt: Target | None = None, cov_src=None, cov_tgt=None, pair_order=None, exact=False,
         **prm):
    """computeTransformation (:381-514).  pair_order: None (index order), "reversed", or a seed for a random permutation
    of each iteration's pairs.  Returns final (f32 4x4), converged, state, iterations, f, pairs, evaluations and the
    per-iteration history (T, pairs, f, inner, evals, status, delta, state, index, d2, x0 and the trial points)."""
    p = dict(DEFAULTS)
    p.update(prm)
    tgt = Target(target) if tgt is None else tgt
    guess = np.eye(4, dtype=F32) if guess is None else np.asarray(guess, F32)
    k = p["k_correspondences"]
    if cov_tgt is None:
        cov_tgt = covariances(tgt.pts, k, p["gicp_epsilon"])[0]
    if cov_src is None:
        cov_src = covariances(source, k, p["gicp_epsilon"])[0]
    trans = np.eye(4, dtype=F32)
    prev = trans.copy()
    iterations, evals_total = 0, 0
    converged, state, f_last, n_pairs = False, NOT_CONVERGED, 0.0, 0
    hist = []
    while not converged:
        pr = Pairs(source, tgt, guess, trans, cov_src, cov_tgt, p["max_corr_dist"], exact)
        n_pairs = pr.m
        prev = trans.copy()
        rec = {"T": trans.copy(), "pairs": pr.m, "f": 0.0, "inner": 0, "evals": 0, "status": MIN_RUNNING, "delta": 0.0,
               "index": pr.index, "d2": pr.d2, "ties": pr.ties, "trials": [], "pair_set": pr}
        hist.append(rec)
        if pr.m < 4:
            state = rec["state"] = NO_CORRESPONDENCES
            break
        if pair_order is None:
            order = None
        elif isinstance(pair_order, str):
            order = np.arange(pr.m)[::-1]
        else:
            order = np.random.default_rng(pair_order + iterations).permutation(pr.m)
        x0 = state_of_transform(trans)
        x, f, status, inner, trials = solve(pr, x0, p["max_inner_iter"], pair_order=order)
        evals_total += len(trials)
        rec.update(f=f, inner=inner, evals=len(trials), status=status, trials=trials, x0=x0, x=x)
        f_last = f
        if status == MIN_FAILED:
            state = rec["state"] = SOLVER_FAILED
            break
        trans = apply_state(np.eye(4, dtype=F32), x)
        delta = 0.0
        for a in range(4):
            for b in range(4):
                ratio = 1.0 / p["rot_eps"] if (a < 3 and b < 3) else 1.0 / p["trans_eps"]
                delta = max(delta, ratio * abs(float(prev[a, b] - trans[a, b])))  # an f32 difference
        iterations += 1
        rec.update(T=trans.copy(), delta=delta)
        if iterations >= p["max_iter"] or delta < 1.0:
            converged = True
            state = ITERATIONS if iterations >= p["max_iter"] else DELTA
            prev = trans.copy()
        rec["state"] = state
    return {"final": final_of(prev, guess), "converged": converged, "state": state, "iterations": iterations, "f": f_last,
            "pairs": n_pairs, "evals": evals_total, "history": hist}
