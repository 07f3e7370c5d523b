"""Absolute and relative pose error of a trajectory against a reference one (host numpy), the two figures the
reference README judges a map by.  A trajectory is a TUM array, (n, 8) rows `time x y z qx qy qz qw`, or the path of a
file of such lines (what write_tum writes).  Poses are associated by time: every pose of the estimate goes with the
reference pose nearest in time, and the pair counts when the two stamps differ by at most max_diff seconds."""
from __future__ import annotations

import numpy as np

__all__ = ["ape", "rpe", "read_tum", "associate", "umeyama", "path_length"]


def read_tum(traj) -> np.ndarray:
    """(n, 8) f64 from a TUM array or a file path."""
    a = np.loadtxt(traj, dtype=np.float64, ndmin=2) if isinstance(traj, (str, bytes)) or hasattr(traj, "__fspath__") else np.asarray(traj, np.float64)
    if a.size == 0:
        return np.zeros((0, 8))
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("a trajectory is (n, 8) rows time x y z qx qy qz qw")
    return a


def path_length(traj) -> float:
    """The summed distance between consecutive positions."""
    p = read_tum(traj)[:, 1:4]
    return float(np.sqrt((np.diff(p, axis=0) ** 2).sum(1)).sum())


def associate(estimate, reference, max_diff: float = 0.01):
    """(indices into the estimate, indices into the reference) of the associated pairs, in the estimate's order; the
    earlier of two equally near reference stamps is taken."""
    te, tr = read_tum(estimate)[:, 0], read_tum(reference)[:, 0]
    if len(te) == 0 or len(tr) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.argsort(tr, kind="stable")
    ts = tr[order]
    hi = np.clip(np.searchsorted(ts, te), 1, len(ts) - 1) if len(ts) > 1 else np.zeros(len(te), np.int64)
    lo = np.maximum(hi - 1, 0)
    pick = np.where(np.abs(ts[lo] - te) <= np.abs(ts[hi] - te), lo, hi)
    keep = np.abs(ts[pick] - te) <= max_diff
    return np.flatnonzero(keep), order[pick[keep]]


def umeyama(src: np.ndarray, dst: np.ndarray):
    """The rigid motion (R, t), no scale, that minimises sum |R src_i + t - dst_i|^2 (Umeyama 1991)."""
    ms, md = src.mean(0), dst.mean(0)
    U, _, Vt = np.linalg.svd((dst - md).T @ (src - ms))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt)) or 1.0])
    R = U @ S @ Vt
    return R, md - R @ ms


def _matrices(rows: np.ndarray) -> np.ndarray:
    q = rows[:, 4:8] / np.linalg.norm(rows[:, 4:8], axis=1, keepdims=True)
    x, y, z, w = q.T
    T = np.zeros((len(rows), 4, 4))
    T[:, 0, 0], T[:, 0, 1], T[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    T[:, 1, 0], T[:, 1, 1], T[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    T[:, 2, 0], T[:, 2, 1], T[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    T[:, :3, 3] = rows[:, 1:4]
    T[:, 3, 3] = 1.0
    return T


def _stats(err: np.ndarray) -> dict:
    if len(err) == 0:
        return {"rmse": float("nan"), "mean": float("nan"), "max": float("nan")}
    return {"rmse": float(np.sqrt((err ** 2).mean())), "mean": float(err.mean()), "max": float(err.max())}


def ape(estimate, reference, align: bool = True, max_diff: float = 0.01) -> dict:
    """Absolute pose error, translation part: |p_est - p_ref| over the associated pairs, after the rigid Umeyama
    alignment of the estimate onto the reference when align is set (at least three pairs).  Returns rmse, mean, max (m),
    matched (pairs) and path_length (of the whole reference trajectory, m)."""
    est, ref = read_tum(estimate), read_tum(reference)
    ie, ir = associate(est, ref, max_diff)
    pe, pr = est[ie, 1:4], ref[ir, 1:4]
    if align and len(ie) >= 3:
        R, t = umeyama(pe, pr)
        pe = pe @ R.T + t
    out = _stats(np.sqrt(((pe - pr) ** 2).sum(1)))
    out.update(matched=int(len(ie)), path_length=path_length(ref))
    return out


def rpe(estimate, reference, max_diff: float = 0.01) -> dict:
    """Relative pose error over consecutive associated pairs, translation part: with Q the reference and P the
    estimate, |trans((Q_i^-1 Q_i+1)^-1 (P_i^-1 P_i+1))|.  Returns rmse, mean, max (m) and matched (relative pairs)."""
    est, ref = read_tum(estimate), read_tum(reference)
    ie, ir = associate(est, ref, max_diff)
    P, Q = _matrices(est[ie]), _matrices(ref[ir])
    if len(ie) < 2:
        return dict(_stats(np.zeros(0)), matched=0)
    dP = np.linalg.inv(P[:-1]) @ P[1:]
    dQ = np.linalg.inv(Q[:-1]) @ Q[1:]
    E = np.linalg.inv(dQ) @ dP
    out = _stats(np.sqrt((E[:, :3, 3] ** 2).sum(1)))
    out["matched"] = int(len(ie) - 1)
    return out
