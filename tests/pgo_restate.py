"""numpy / scipy restatement of the pose-graph optimiser (DESIGN.md §2 "Pose graph"): the model of what pgo_node asks
GTSAM for, solved as a batch problem.  The device (csrc/posegraph.hip) is compared against this file.

Variables: one SE(3) pose per keyframe (4x4, f64).  Tangent order [wx wy wz vx vy vz]; retraction X <- X Exp(d).
Factors: a prior on node 0, residual Log(P^-1 X0); between factors (i, j, Z, var[6], k), residual
e = Log(Z^-1 Xi^-1 Xj) (the full SE(3) logarithm), whitened by 1/sqrt(var); Cauchy weight w = k^2 / (k^2 + |e|^2_S) and
cost k^2/2 log(1 + |e|^2_S / k^2) where k > 0, Gaussian (w = 1, cost |e|^2_S / 2) where k == 0.
Solution: iteratively reweighted Gauss-Newton with the exact Jacobians de/ddj = Jr^-1(e), de/ddi = -Jr^-1(e) Ad(Xj^-1 Xi),
until max|d| < step_eps.  Two linear solves: dense lstsq on the whitened Jacobian (QR) and scipy.sparse normal equations.

Every function takes stacked inputs (leading axes are batch axes).
"""
import math

import numpy as np

SERIES_BELOW = 0.2      # |w| below which the coefficient functions use their power series
PI_MARGIN = 1e-6        # residual rotations closer to pi than this are rejected
PRIOR_VAR = (1e-12,) * 6
ODOM_VAR = (1e-6,) * 3 + (1e-4,) * 3


def _horner(t, coef):
    out = np.full_like(t, coef[-1])
    for c in coef[-2::-1]:
        out = out * t + c
    return out


# power series in t = theta^2, six terms each
_SA = [1.0, -1 / 6, 1 / 120, -1 / 5040, 1 / 362880, -1 / 39916800]                       # sin(th)/th
_SB = [1 / 2, -1 / 24, 1 / 720, -1 / 40320, 1 / 3628800, -1 / 479001600]                # (1 - cos)/th^2
_SC = [1 / 6, -1 / 120, 1 / 5040, -1 / 362880, 1 / 39916800, -1 / 6227020800]           # (th - sin)/th^3
_SD = [1 / 12, 1 / 720, 1 / 30240, 1 / 1209600, 1 / 47900160, 691 / 1307674368000]      # (1 - th/2 cot(th/2))/th^2
_SE = [1 / 24, -1 / 720, 1 / 40320, -1 / 3628800, 1 / 479001600, -1 / 87178291200]      # (th^2/2 + cos - 1)/th^4
_SF = [1 / 120, -2 / 5040, 3 / 362880, -4 / 39916800, 5 / 6227020800, -6 / 1307674368000]  # (2th + th cos - 3 sin)/(2 th^5)


def coefficients(theta):
    """A, B, C, D, E, F of the table above at theta >= 0 (series below SERIES_BELOW, closed forms from there on)."""
    th = np.asarray(theta, np.float64)
    t = th * th
    small = th < SERIES_BELOW
    ths = np.where(small, 1.0, th)
    s, c = np.sin(ths), np.cos(ths)
    t1 = ths * ths
    half = 0.5 * ths
    closed = (s / ths, (1 - c) / t1, (ths - s) / (t1 * ths), (1 - half * np.cos(half) / np.sin(half)) / t1,
              (0.5 * t1 + c - 1) / (t1 * t1), (2 * ths + ths * c - 3 * s) / (2 * t1 * t1 * ths))
    return tuple(np.where(small, _horner(t, ser), cl) for ser, cl in zip((_SA, _SB, _SC, _SD, _SE, _SF), closed))


def hat(w):
    w = np.asarray(w, np.float64)
    out = np.zeros(w.shape[:-1] + (3, 3))
    out[..., 0, 1], out[..., 0, 2] = -w[..., 2], w[..., 1]
    out[..., 1, 0], out[..., 1, 2] = w[..., 2], -w[..., 0]
    out[..., 2, 0], out[..., 2, 1] = -w[..., 1], w[..., 0]
    return out


def _poly(w, a, b):
    """I + a W + b W^2"""
    W = hat(w)
    return np.eye(3) + a[..., None, None] * W + b[..., None, None] * (W @ W)


def exp_se3(xi):
    xi = np.asarray(xi, np.float64)
    w, v = xi[..., :3], xi[..., 3:]
    A, B, Cc, _, _, _ = coefficients(np.linalg.norm(w, axis=-1))
    T = np.zeros(xi.shape[:-1] + (4, 4))
    T[..., :3, :3] = _poly(w, A, B)
    T[..., :3, 3] = (_poly(w, B, Cc) @ v[..., None])[..., 0]
    T[..., 3, 3] = 1.0
    return T


class RotationNearPi(ValueError):
    pass


def log_so3(R):
    a = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = np.linalg.norm(a, axis=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    th = np.arctan2(s, c)
    if np.any(th > math.pi - PI_MARGIN):
        raise RotationNearPi("residual rotation within 1e-6 of pi")
    small = th < SERIES_BELOW
    f = np.where(small, 1.0 / coefficients(th)[0], th / np.where(small, 1.0, s))
    return a * f[..., None]


def log_se3(T):
    T = np.asarray(T, np.float64)
    w = log_so3(T[..., :3, :3])
    D = coefficients(np.linalg.norm(w, axis=-1))[3]
    v = (_poly(w, np.full_like(D, -0.5), D) @ T[..., :3, 3:4])[..., 0]
    return np.concatenate([w, v], -1)


def q_right(xi):
    """The lower-left block of the right Jacobian of SE(3) (GTSAM's computeQforExpmapDerivative; Barfoot's Q at -xi)."""
    w, v = xi[..., :3], xi[..., 3:]
    _, _, Cc, _, E, F = coefficients(np.linalg.norm(w, axis=-1))
    W, V = hat(w), hat(v)
    WV, VW = W @ V, V @ W
    WVW = WV @ W
    Cc, E, F = Cc[..., None, None], E[..., None, None], F[..., None, None]
    return -0.5 * V + Cc * (WV + VW - WVW) - E * (W @ WV + VW @ W - 3 * WVW) + F * (WVW @ W + W @ WVW)


def jr(xi):
    xi = np.asarray(xi, np.float64)
    w = xi[..., :3]
    _, B, Cc, _, _, _ = coefficients(np.linalg.norm(w, axis=-1))
    Jw = _poly(w, -B, Cc)
    J = np.zeros(xi.shape[:-1] + (6, 6))
    J[..., :3, :3] = Jw
    J[..., 3:, 3:] = Jw
    J[..., 3:, :3] = q_right(xi)
    return J


def jr_inv(xi):
    """The closed-form inverse right Jacobian of SE(3): Log(T Exp(d)) = Log(T) + Jr^-1(Log T) d + O(d^2)."""
    xi = np.asarray(xi, np.float64)
    w = xi[..., :3]
    D = coefficients(np.linalg.norm(w, axis=-1))[3]
    Ji = _poly(w, np.full_like(D, 0.5), D)
    J = np.zeros(xi.shape[:-1] + (6, 6))
    J[..., :3, :3] = Ji
    J[..., 3:, 3:] = Ji
    J[..., 3:, :3] = -Ji @ q_right(xi) @ Ji
    return J


def inv_se3(T):
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def adjoint(T):
    T = np.asarray(T, np.float64)
    R = T[..., :3, :3]
    out = np.zeros(T.shape[:-2] + (6, 6))
    out[..., :3, :3] = R
    out[..., 3:, 3:] = R
    out[..., 3:, :3] = hat(T[..., :3, 3]) @ R
    return out


def rpy(T):
    """GTSAM's Rot3::rpy of the poses' rotations (what keyframePosesUpdated receives), with the translations: (n, 6)
    x y z roll pitch yaw."""
    T = np.asarray(T, np.float64)
    R = T[..., :3, :3]
    return np.stack([T[..., 0, 3], T[..., 1, 3], T[..., 2, 3], np.arctan2(R[..., 2, 1], R[..., 2, 2]),
                     np.arctan2(-R[..., 2, 0], np.hypot(R[..., 2, 1], R[..., 2, 2])), np.arctan2(R[..., 1, 0], R[..., 0, 0])], -1)


class Graph:
    """The factor graph as ndt_pgo holds it: add_node gives node 0 the prior and every later node the odometry edge
    from its predecessor, computed from the two given poses."""

    def __init__(self, prior_var=PRIOR_VAR, odom_var=ODOM_VAR):
        self.prior_var = np.asarray(prior_var, np.float64)
        self.odom_var = np.asarray(odom_var, np.float64)
        self.init = []      # the poses as given
        self.ei, self.ej, self.Z, self.var, self.k, self.odom = [], [], [], [], [], []

    def __len__(self):
        return len(self.init)

    def add_node(self, pose):
        P = np.array(pose, np.float64).reshape(4, 4)
        if self.init:
            self.add_between(len(self.init) - 1, len(self.init), inv_se3(self.init[-1]) @ P, self.odom_var, 0.0, odom=True)
        self.init.append(P)
        return len(self.init) - 1

    def add_between(self, i, j, Z, var, robust_k=1.0, odom=False):
        if not odom and (i == j or not (0 <= i < len(self.init) and 0 <= j < len(self.init))):
            raise ValueError("bad edge")
        self.ei.append(i)
        self.ej.append(j)
        self.Z.append(np.array(Z, np.float64).reshape(4, 4))
        self.var.append(np.broadcast_to(np.asarray(var, np.float64), (6,)).copy())
        self.k.append(float(robust_k))
        self.odom.append(odom)

    # ---------------------------------------------------------------------------------------------- evaluation
    def _arrays(self):
        return (np.array(self.ei, int), np.array(self.ej, int), np.array(self.Z).reshape(-1, 4, 4),
                np.array(self.var).reshape(-1, 6), np.array(self.k))

    def residuals(self, poses):
        """(e_prior (6,), e_edges (m, 6)) unwhitened."""
        X = np.asarray(poses, np.float64)
        ei, ej, Z, _, _ = self._arrays()
        e0 = log_se3(inv_se3(self.init[0]) @ X[0])
        e = log_se3(inv_se3(Z) @ inv_se3(X[ei]) @ X[ej]) if len(ei) else np.zeros((0, 6))
        return e0, e

    def _robust(self, e):
        _, _, _, var, k = self._arrays()
        s = np.sum(e * e / var, -1) if len(e) else np.zeros(0)
        k2 = np.where(k > 0, k * k, 1.0)
        w = np.where(k > 0, k2 / (k2 + s), 1.0)
        rho = np.where(k > 0, 0.5 * k2 * np.log1p(s / k2), 0.5 * s)
        return s, w, rho

    def weights(self, poses):
        """The robust weight of every between edge that is not an odometry edge, in the order they were added."""
        _, e = self.residuals(poses)
        return self._robust(e)[1][~np.array(self.odom, bool)]

    def cost(self, poses):
        e0, e = self.residuals(poses)
        return float(0.5 * np.sum(e0 * e0 / self.prior_var) + np.sum(self._robust(e)[2]))

    def linearize(self, poses):
        """Row blocks of the whitened, weighted system: (rows (m+1, 6), Ji (m+1, 6, 6), Jj (m+1, 6, 6), i, j); block 0 is
        the prior (its Jj acts on node 0, its Ji is unused)."""
        X = np.asarray(poses, np.float64)
        ei, ej, _, var, _ = self._arrays()
        e0, e = self.residuals(X)
        _, w, _ = self._robust(e)
        scale = np.concatenate([1.0 / np.sqrt(self.prior_var)[None], np.sqrt(w)[:, None] / np.sqrt(var)], 0)
        E = np.concatenate([e0[None], e], 0)
        Jj = jr_inv(E)
        Ji = np.zeros_like(Jj)
        if len(ei):
            Ji[1:] = -Jj[1:] @ adjoint(inv_se3(X[ej]) @ X[ei])
        i = np.concatenate([[0], ei])
        j = np.concatenate([[0], ej])
        return E * scale, Ji * scale[..., None], Jj * scale[..., None], i, j

    def gn_step_at(self, poses, solver="lstsq"):
        """The Gauss-Newton step (n, 6) of the reweighted problem linearised at poses."""
        n = len(poses)
        r, Ji, Jj, i, j = self.linearize(poses)
        m = len(r)
        if solver == "lstsq":
            A = np.zeros((m, 6, n, 6))
            A[np.arange(m), :, j, :] = Jj
            A[np.arange(1, m), :, i[1:], :] = Ji[1:]
            d = np.linalg.lstsq(A.reshape(6 * m, 6 * n), -r.reshape(-1), rcond=None)[0]
        elif solver == "sparse":
            import scipy.sparse as sp
            import scipy.sparse.linalg as spl
            rows = (6 * np.arange(m)[:, None, None] + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), int)
            colj = (6 * j[:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), int)
            coli = (6 * i[1:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), int)
            A = sp.csr_matrix((np.concatenate([Jj.ravel(), Ji[1:].ravel()]),
                               (np.concatenate([rows.ravel(), rows[1:].ravel()]), np.concatenate([colj.ravel(), coli.ravel()]))),
                              shape=(6 * m, 6 * n))
            d = spl.spsolve((A.T @ A).tocsc(), -(A.T @ r.reshape(-1)))
        else:
            raise ValueError(solver)
        return d.reshape(n, 6)

    def optimize(self, poses=None, solver="lstsq", step_eps=1e-10, max_iter=100):
        """IRLS Gauss-Newton from poses (default: the poses as given).  Returns (poses, info)."""
        X = np.array(self.init if poses is None else poses, np.float64)
        hist, step = [], math.inf
        cost0 = self.cost(X)
        for _ in range(max_iter):
            c = self.cost(X)
            d = self.gn_step_at(X, solver)
            X = X @ exp_se3(d)
            step = float(np.max(np.abs(d)))
            hist.append((c, step))
            if step < step_eps:
                break
        return X, {"iterations": len(hist), "converged": step < step_eps, "cost0": cost0, "cost": self.cost(X), "max_step": step,
                   "history": hist}


def build(poses, loops, **kw):
    """A Graph of 4x4 poses and loops [(i, j, Z, var, k)]."""
    g = Graph(**kw)
    for P in poses:
        g.add_node(P)
    for i, j, Z, var, k in loops:
        g.add_between(i, j, Z, var, k)
    return g
