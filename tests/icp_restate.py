"""numpy / scipy restatement of the point-to-point ICP semantics the device implements (ICP section: PCL 1.7's
IterativeClosestPoint + CorrespondenceEstimation + TransformationEstimationSVD + DefaultConvergenceCriteria as
pgo_node's ICPRefine drives them; PCL itself is not available, so this restatement is the specification's executable
form — parity with PCL unpinned).

Differences from the device are confined to f64 summation order and the SVD routine: the correspondence is the device's
by construction (the tree only proposes candidates, the f32 L2_Simple value and the tie rule decide), transforms are f32
with the device's operation order, sums are two-pass demeaned f64, the SVD is numpy's.
"""
import os

import numpy as np
from scipy.spatial import cKDTree

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
STATE_NAMES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")
DBL_MAX = float(np.finfo(np.float64).max)
F32 = np.float32
WORKERS = min(16, os.cpu_count() or 1)  # tree query threads


def transform_f32(T, X):
    """pcl::transformPointCloud in f32: ((T0 x + T4 y) + T8 z) + T12 per row, no fused multiply-add."""
    T = np.asarray(T, F32)
    X = np.asarray(X, F32)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    out = np.empty((len(X), 3), F32)
    for a in range(3):
        out[:, a] = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
    return out


def mat4_mul_f32(A, B):
    """Matrix4f product with each entry summed in order: ((a0 b0 + a1 b1) + a2 b2) + a3 b3."""
    A = np.asarray(A, F32)
    B = np.asarray(B, F32)
    C = np.empty((4, 4), F32)
    for i in range(4):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


def l2_simple_f32(t, q):
    """FLANN L2_Simple in f32: (dx^2 + dy^2) + dz^2 (t - q, as the device orders the subtraction)."""
    u = (np.asarray(t, F32) - np.asarray(q, F32)).astype(F32)
    return ((u[..., 0] * u[..., 0]) + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]


class Target:
    def __init__(self, target):
        self.pts = np.ascontiguousarray(np.asarray(target, F32)[:, :3])
        self.tree = cKDTree(self.pts.astype(np.float64)) if len(self.pts) else None


def nearest_bruteforce(X, P, chunk_pairs: int = 1 << 22):
    """Nearest point of P for every query of X over every pair (no tree, no candidate list): the f32 L2_Simple value of
    each pair, in chunks of queries.  Returns (the lowest index of P at the minimum, the minimum as f32, the number of
    points of P at the minimum).  Exact under any number of ties, which the k-nearest re-ranking of `correspondences`
    is not: k candidates at one distance can crowd the lowest index out of the list."""
    X = np.ascontiguousarray(np.asarray(X, F32)[:, :3])
    P = np.ascontiguousarray(np.asarray(P, F32)[:, :3])
    n, m = len(X), len(P)
    if m == 0 or n == 0:
        return np.full(n, -1, np.int64), np.full(n, np.inf, F32), np.zeros(n, np.int64)
    idx = np.empty(n, np.int64)
    best = np.empty(n, F32)
    count = np.empty(n, np.int64)
    rows = max(1, chunk_pairs // m)
    for s in range(0, n, rows):
        d2 = l2_simple_f32(P[None, :, :], X[s:s + rows, None, :])
        b = d2.min(1)
        at = d2 == b[:, None]
        idx[s:s + rows] = at.argmax(1)  # the first True: the lowest index
        best[s:s + rows] = b
        count[s:s + rows] = at.sum(1)
    return idx, best, count


def correspondences(X, tgt: Target, k: int = 4, exact: bool = False):
    """Nearest target point of every query: the tree's k nearest re-ranked by the f32 L2_Simple value, equal values to
    the lowest target index.  Returns (index, d2 as f32, queries with two candidates at an equal f32 distance).
    exact: every pair instead (nearest_bruteforce); the flags are then the queries with two or more target points at
    the minimum."""
    X = np.asarray(X, F32)
    n, m = len(X), len(tgt.pts)
    if m == 0 or n == 0:
        return np.full(n, -1, np.int64), np.full(n, np.inf, F32), np.zeros(n, bool)
    if exact:
        idx, best, count = nearest_bruteforce(X, tgt.pts)
        return idx, best, count > 1
    k = min(k, m)
    _, ii = tgt.tree.query(X.astype(np.float64), k=k, workers=WORKERS)
    ii = ii.reshape(n, k)
    d2 = l2_simple_f32(tgt.pts[ii], X[:, None, :])
    best = d2.min(1)
    at_best = d2 == best[:, None]
    idx = np.where(at_best, ii, m).min(1)
    # any two candidates of a query at the same f32 distance (not only at the minimum): the input condition of the
    # exact-match tests
    srt = np.sort(d2, 1)
    ties = (srt[:, 1:] == srt[:, :-1]).any(1) if k > 1 else np.zeros(n, bool)
    return idx, best.astype(F32), ties


def umeyama(P, Q, dtype=np.float64):
    """Rigid transform P -> Q without scale (TransformationEstimationSVD / Eigen::umeyama), two-pass f64, as f32 4x4.
    dtype=np.longdouble evaluates the means, the cross-covariance and the translation in extended precision (the SVD
    stays LAPACK's f64 one): the yardstick for how much of `final` is the estimate's own rounding."""
    P = np.asarray(P, dtype)
    Q = np.asarray(Q, dtype)
    pm, qm = P.mean(0), Q.mean(0)
    sigma = (Q - qm).T @ (P - pm) / len(P)
    U, _, Vt = np.linalg.svd(sigma.astype(np.float64))
    s = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = (U @ np.diag([1.0, 1.0, s]) @ Vt).astype(dtype)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = R
    T[:3, 3] = qm - R @ pm
    return T.astype(F32)


def icp(source, target, guess=None, max_corr_dist=float(np.sqrt(DBL_MAX)), max_iter=10, trans_eps=0.0, fit_eps=0.0,
        min_pairs=3, k=4, tgt: Target | None = None, exact: bool = False, estimate_dtype=np.float64):
    """align(guess).  Returns final (f32 4x4), converged, state, iterations, mse, pairs and the per-iteration history
    (incremental T, pairs, mse, state, and the iteration's matched index (-1 rejected) / d2 / tie flags).
    exact: correspondences over every pair (exact under ties) instead of the tree's k nearest; estimate_dtype: umeyama's."""
    tgt = Target(target) if tgt is None else tgt
    guess = np.eye(4, dtype=F32) if guess is None else np.asarray(guess, F32)
    final = guess.copy()
    X = np.ascontiguousarray(np.asarray(source, F32)[:, :3])
    if not np.array_equal(guess, np.eye(4, dtype=F32)):
        X = transform_f32(guess, X)
    max_corr2 = float(max_corr_dist) * float(max_corr_dist)
    prev = DBL_MAX
    iterations = 0
    hist = []
    converged, state, mse, pairs = False, NOT_CONVERGED, 0.0, 0
    while True:
        idx, d2, ties = correspondences(X, tgt, k, exact)
        keep = (idx >= 0) & (d2.astype(np.float64) <= max_corr2)
        pairs = int(keep.sum())
        mse = float(d2[keep].astype(np.float64).sum() / pairs) if pairs else 0.0
        rec = {"T": np.eye(4, dtype=F32), "pairs": pairs, "mse": mse, "index": np.where(keep, idx, -1), "d2": d2, "ties": ties}
        hist.append(rec)
        if pairs < min_pairs:
            state, converged = NO_CORRESPONDENCES, False
            rec["state"] = state
            break
        T = umeyama(X[keep], tgt.pts[idx[keep]], estimate_dtype)
        rec["T"] = T
        X = transform_f32(T, X)
        final = mat4_mul_f32(T, final)
        iterations += 1
        Td = T.astype(np.float64)
        cos_angle = 0.5 * ((Td[0, 0] + Td[1, 1] + Td[2, 2]) - 1.0)
        tsq = (Td[0, 3] * Td[0, 3] + Td[1, 3] * Td[1, 3]) + Td[2, 3] * Td[2, 3]
        state = NOT_CONVERGED
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if iterations >= max_iter:
                state = ITERATIONS
            elif trans_eps > 0 and cos_angle >= 1.0 - trans_eps and tsq <= trans_eps:
                state = TRANSFORM
            elif abs(mse - prev) < 1e-12:
                state = ABS_MSE
            elif fit_eps > 0 and np.float64(abs(mse - prev)) / np.float64(prev) < fit_eps:
                state = REL_MSE
            else:
                prev = mse
        rec["state"] = state
        if state != NOT_CONVERGED:
            converged = True
            break
    return {"final": final, "converged": converged, "state": state, "iterations": iterations, "mse": mse, "pairs": pairs,
            "history": hist}


def fitness_score(source, target, T, max_range=DBL_MAX, tgt: Target | None = None):
    """pcl::Registration::getFitnessScore: mean f32 squared nearest distance over those <= max_range (f64 sum)."""
    tgt = Target(target) if tgt is None else tgt
    X = transform_f32(T, np.asarray(source, F32)[:, :3])
    _, d2, _ = correspondences(X, tgt)
    d = d2.astype(np.float64)
    d = d[d <= max_range]
    return float(d.sum() / len(d)) if len(d) else DBL_MAX


def get_transformation(x, y, z, roll, pitch, yaw):
    """pcl::getTransformation in f32 (pcl/common/impl/eigen.hpp)."""
    f = F32
    A, B = np.cos(f(yaw)), np.sin(f(yaw))
    C, D = np.cos(f(pitch)), np.sin(f(pitch))
    E, F = np.cos(f(roll)), np.sin(f(roll))
    DE, DF = D * E, D * F
    t = np.eye(4, dtype=F32)
    t[0] = [A * C, A * DF - B * E, B * F + A * DE, f(x)]
    t[1] = [B * C, A * E + B * DF, B * DE - A * F, f(y)]
    t[2] = [-D, C * F, C * E, f(z)]
    return t
