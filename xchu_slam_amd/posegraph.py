"""Pose-graph optimisation for pgo_node's loop closures, backed by libndt_hip.so (include/ndt_hip.h, ndt_pgo_*; the
kernel is csrc/posegraph.hip).

pgo_node turns every keyframe and every accepted loop into a factor of a GTSAM pose graph and ships the optimised
keyframe poses (pgo_node.cpp:249-291, 453-475, 498-528).  The reference holds no GTSAM source, so this is a model of
what it asks GTSAM for, solved as a batch problem (DESIGN.md "Pose graph", parity unpinned):

    with xa.PoseGraph() as pg:
        for p in keyframe_poses: pg.add_node(p)                 # prior on node 0, odometry edges between neighbours
        for i, j, T, score in accepted: pg.add_loop(i, j, xa.loop_measurement(poses, i, j, T), score)
        info = pg.optimize()
        poses6d = pg.poses6d()

`optimize_loops` does exactly that with what `close_loops` returns.  Under `useGPS` pgo_node also adds a
gtsam::GPSFactor per keyframe that has a fix (pgo_node.cpp:103-111, 168-182, 207-212, 278-287): `pg.add_position(node,
xyz, variances)`, and `gps_factors` builds those from keyframe and fix times.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import synth
from ._ctxobj import _CtxObject
from ._lib import PGO_SOLVER_CG, PGO_SOLVER_DIRECT, PgoParams, PgoRecord, PgoResult, PgoSolverStats, check
from .ndt import NormalDistributionsTransform, _dp

__all__ = ["PoseGraph", "gps_factors", "loop_measurement", "optimize_loops"]

_PARAM_NAMES = tuple(k for k, _ in PgoParams._fields_)
_SOLVERS = {"cg": PGO_SOLVER_CG, "direct": PGO_SOLVER_DIRECT}
_SOLVER_NAMES = {v: k for k, v in _SOLVERS.items()}


def _pose44(pose) -> np.ndarray:
    p = np.asarray(pose, np.float64)
    if p.shape == (6,):
        return synth.pose_matrix(*p)
    if p.shape != (4, 4):
        raise ValueError("a pose is a 4 x 4 matrix or (x, y, z, roll, pitch, yaw)")
    return p


def _colmajor(T: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(T.T).reshape(-1)


def _inv(T: np.ndarray) -> np.ndarray:
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


class PoseGraph(_CtxObject):
    """The pose graph of pgo_node on MI355X.  It runs on a registration context: its own, or the one of an existing
    NormalDistributionsTransform (`registration=`), whose device and stream it then shares.  **params are
    ndt_pgo_params fields: max_iter, step_eps, cg_max_iter, cg_rtol, prior_var, odom_var.  solver: the linear solver
    of each Gauss-Newton step, "cg" (conjugate gradients inside one launch, the default) or "direct" (the dense loop-space
    factorisation of csrc/posegraph_direct.hip; at most 6 loops + 3 positions = 8192 rows)."""

    _DESTROY = "ndt_pgo_destroy"
    _WHAT = "pose-graph"

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None, solver="cg", **params):
        super().__init__(device, registration)

        def six(k, v):  # a variance: one value for all six components, or six
            return (C.c_double * 6)(*np.broadcast_to(np.asarray(v, np.float64), (6,))) if k.endswith("_var") else v

        self._params = self._default_params(PgoParams, "ndt_pgo_default_params", params, six)
        pg = C.c_void_p()
        check(self._lib.ndt_pgo_create(self.ctx, C.byref(self._params), C.byref(pg)), self.ctx)
        self._handle = pg
        if solver != "cg":
            try:
                self.set_solver(solver)
            except Exception:
                self.close()
                raise

    def set_solver(self, solver):
        """The linear solver of later optimize() calls: "cg" or "direct" (or the C ABI's NDT_PGO_SOLVER_* value)."""
        if isinstance(solver, str):
            if solver not in _SOLVERS:
                raise ValueError("solver is 'cg' or 'direct'")
            solver = _SOLVERS[solver]
        check(self._lib.ndt_pgo_set_solver(self._handle, int(solver)), self.ctx)

    @property
    def solver(self) -> str:
        return _SOLVER_NAMES[int(self._lib.ndt_pgo_get_solver(self._handle))]

    def solver_stats(self) -> dict:
        """Of the last optimize(): the solver it used, d = 6 loops + 3 positions, and under "direct" the tile width, the
        number of factorisations and whether a refinement pass ran."""
        st = PgoSolverStats()
        check(self._lib.ndt_pgo_solver_stats(self._handle, C.byref(st)), self.ctx)
        return {"solver": _SOLVER_NAMES[int(st.solver)], "d": int(st.d), "tile": int(st.tile),
                "factorizations": int(st.factorizations), "refined": bool(st.refined)}

    def __len__(self) -> int:
        return int(self._lib.ndt_pgo_size(self._handle))

    def params(self) -> dict:
        return {k: (list(getattr(self._params, k)) if k.endswith("_var") else getattr(self._params, k)) for k in _PARAM_NAMES}

    # ------------------------------------------------------------------ the graph
    def add_node(self, pose) -> int:
        """A keyframe pose (4 x 4, or (x, y, z, roll, pitch, yaw) through Pose6D2Matrix).  Node 0 gets the prior, every
        later node the odometry edge from its predecessor; the pose is the node's initial estimate."""
        idx = C.c_int()
        check(self._lib.ndt_pgo_add_node(self._handle, _dp(_colmajor(_pose44(pose))), C.byref(idx)), self.ctx)
        return idx.value

    def set_estimate(self, node: int, pose):
        """The estimate of a stored node replaced by `pose` (as add_node takes it); host state only, no factor changes."""
        check(self._lib.ndt_pgo_set_estimate(self._handle, int(node), _dp(_colmajor(_pose44(pose)))), self.ctx)

    def add_loop(self, i: int, j: int, Z, variances, robust_k: float = 1.0):
        """BetweenFactor(i, j, Z): variances is one number (pgo_node uses the ICP fitness score for all six) or six;
        robust_k the Cauchy kernel's width (pgo_node: 1; 0: Gaussian)."""
        var = np.ascontiguousarray(np.broadcast_to(np.asarray(variances, np.float64), (6,)))
        check(self._lib.ndt_pgo_add_between(self._handle, int(i), int(j), _dp(_colmajor(_pose44(Z))), _dp(var), float(robust_k)), self.ctx)

    def add_position(self, node: int, xyz, variances, robust_k: float = 1.0):
        """GPSFactor(node, xyz): the node's translation measured as xyz (metres, map frame); variances is one number
        or three (pgo_node: 1e9, 1e9, 250 - altitude only); robust_k as for add_loop."""
        p = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1))
        if p.shape != (3,):
            raise ValueError("a position is (x, y, z)")
        var = np.ascontiguousarray(np.broadcast_to(np.asarray(variances, np.float64), (3,)))
        check(self._lib.ndt_pgo_add_position(self._handle, int(node), _dp(p), _dp(var), float(robust_k)), self.ctx)

    def optimize(self) -> dict:
        """One optimisation from the current estimate (a later call is a warm start)."""
        r = PgoResult()
        check(self._lib.ndt_pgo_optimize(self._handle, C.byref(r)), self.ctx)
        return {"iterations": int(r.iterations), "converged": bool(r.converged), "cost0": float(r.cost0), "cost": float(r.cost),
                "max_step": float(r.max_step), "cg_iterations": int(r.cg_iterations)}

    def poses(self) -> np.ndarray:
        """The current estimate, (n, 4, 4) f64."""
        n = len(self)
        buf = np.empty(max(1, n) * 16, np.float64)
        check(self._lib.ndt_pgo_get_poses(self._handle, _dp(buf), n, None), self.ctx)
        return buf[:n * 16].reshape(n, 4, 4).transpose(0, 2, 1).copy()

    def poses6d(self) -> np.ndarray:
        """(n, 6) x, y, z, roll, pitch, yaw with the angles as GTSAM's Rot3::rpy gives them, which is what
        keyframePosesUpdated receives (pgo_node.cpp:517-526)."""
        return _poses6d(self.poses())

    def weights(self) -> np.ndarray:
        """The final robust weight of every loop factor of the last optimize(), in the order they were added."""
        n = C.c_int()
        check(self._lib.ndt_pgo_get_weights(self._handle, None, 0, C.byref(n)), self.ctx)
        buf = np.empty(max(1, n.value), np.float64)
        check(self._lib.ndt_pgo_get_weights(self._handle, _dp(buf), n.value, None), self.ctx)
        return buf[:n.value].copy()

    def position_weights(self) -> np.ndarray:
        """The final robust weight of every position factor of the last optimize(), in the order they were added."""
        n = C.c_int()
        check(self._lib.ndt_pgo_get_position_weights(self._handle, None, 0, C.byref(n)), self.ctx)
        buf = np.empty(max(1, n.value), np.float64)
        check(self._lib.ndt_pgo_get_position_weights(self._handle, _dp(buf), n.value, None), self.ctx)
        return buf[:n.value].copy()

    def history(self) -> list[dict]:
        """Per step of the last optimize(): the cost before it, max|d| and the CG iterations it took."""
        n = C.c_int()
        check(self._lib.ndt_pgo_history(self._handle, None, 0, C.byref(n)), self.ctx)
        buf = (PgoRecord * max(1, n.value))()
        check(self._lib.ndt_pgo_history(self._handle, buf, n.value, None), self.ctx)
        return [{"cost": float(buf[i].cost), "max_step": float(buf[i].max_step), "cg_iterations": int(buf[i].cg_iterations)}
                for i in range(n.value)]


def _poses6d(T: np.ndarray) -> np.ndarray:
    """(n, 4, 4) -> (n, 6) x, y, z and GTSAM's Rot3::rpy."""
    R = T[:, :3, :3]
    return np.stack([T[:, 0, 3], T[:, 1, 3], T[:, 2, 3], np.arctan2(R[:, 2, 1], R[:, 2, 2]),
                     np.arctan2(-R[:, 2, 0], np.hypot(R[:, 2, 1], R[:, 2, 2])), np.arctan2(R[:, 1, 0], R[:, 0, 0])], -1)


def _matrix_to_pose6d(T: np.ndarray):
    """Matrix2Pose6D (common.h:51-63): tf's getRPY of the rotation."""
    R = T[:3, :3]
    if abs(R[2, 0]) >= 1.0:   # gimbal lock: tf's first solution, yaw 0
        roll, pitch, yaw = math.atan2(R[2, 1], R[2, 2]), math.copysign(math.pi / 2, -R[2, 0]), 0.0
    else:
        pitch = -math.asin(R[2, 0])
        cp = math.cos(pitch)
        roll = math.atan2(R[2, 1] / cp, R[2, 2] / cp)
        yaw = math.atan2(R[1, 0] / cp, R[0, 0] / cp)
    return T[0, 3], T[1, 3], T[2, 3], roll, pitch, yaw


def loop_measurement(poses, loop_idx: int, curr_idx: int, T_icp, literal_measurement: bool = False) -> np.ndarray:
    """The 4 x 4 measurement Z of BetweenFactor(loop_idx, curr_idx, Z) for an ICP result T_icp (host numpy).

    pgo_node's two clouds were already moved into the map frame with the current poses, so T_icp is a correction of
    the current keyframe's pose, not a relative pose.  The default is the relative pose that correction implies,
    Z = X_loop^-1 T_icp X_curr.  literal_measurement=True is what the reference adds (pgo_node.cpp:465-473):
    Z = T_icp^-1 after Matrix2Pose6D / Pose6D2Pose3."""
    T = np.asarray(T_icp, np.float64)
    if T.shape != (4, 4):
        raise ValueError("T_icp is a 4 x 4 matrix")
    if literal_measurement:
        return _inv(synth.pose_matrix(*_matrix_to_pose6d(T)))
    return _inv(_pose44(poses[loop_idx])) @ T @ _pose44(poses[curr_idx])


def gps_factors(keyframe_times, poses, gps_times, altitudes, eps: float = 0.1, altitude_var: float = 250.0, xy_var: float = 1e9):
    """pgo_node's GPS factors for a replay (host numpy): [(node, xyz (3,), var (3,))] for add_position / optimize_loops.

    The rule of pgo_node.cpp:168-182, 207-212, 278-287 stated as what it means (its queue handling returns with the mutex
    held on a match and its own comment calls GPS not usable yet, so the intent is restated, not the code path): keyframe
    k has GPS iff its nearest fix in time is strictly within eps seconds (an equal distance goes to the earlier fix); the
    altitude offset is the altitude of the first keyframe that has GPS; the constraint is (x, y of that keyframe's pose,
    altitude - offset) with variances (xy_var, xy_var, altitude_var): only the altitude is constrained.  The reference
    takes x and y from recentOptimizedX/Y, the last optimised pose rather than this keyframe's; at a variance of 1e9 the
    difference is far below the solver's step (modelled).  Altitudes are metres; a NavSatFix's latitude and longitude
    are not used."""
    kt = np.asarray(keyframe_times, np.float64).reshape(-1)
    gt = np.asarray(gps_times, np.float64).reshape(-1)
    alt = np.asarray(altitudes, np.float64).reshape(-1)
    if len(poses) != len(kt) or len(gt) != len(alt):
        raise ValueError("one time per keyframe pose and one altitude per fix")
    out, offset = [], None
    if len(gt) == 0:
        return out
    order = np.argsort(gt, kind="stable")       # argmin below then takes the earlier of two equally near fixes
    gt, alt = gt[order], alt[order]
    for k, t in enumerate(kt):
        f = int(np.argmin(np.abs(gt - t)))
        if not abs(gt[f] - t) < eps:
            continue
        if offset is None:
            offset = alt[f]
        P = _pose44(poses[k])
        out.append((k, np.array([P[0, 3], P[1, 3], alt[f] - offset]), np.array([xy_var, xy_var, altitude_var], np.float64)))
    return out


def optimize_loops(poses, accepted, literal_measurement: bool = False, robust_k: float = 1.0, device: int = 0, registration=None,
                   positions=None, solver="cg", **params):
    """pgo_node's back end for a replay: the graph of `poses` (per keyframe a 4 x 4 or (x, y, z, roll, pitch, yaw)) and
    of `accepted` as close_loops returns it ([(loop_idx, curr_idx, transform, score)]; the score is the loop factor's
    variance, as pgo_node.cpp:453-457 has it) and of `positions` ([(node, xyz, var)] as gps_factors returns it, each a
    position factor with robust_k), one optimise with PoseGraph's `solver`.  Returns (poses6d (n, 6), info); info is optimize()'s dict plus
    "weights", "position_weights" and "poses" (n, 4, 4)."""
    with PoseGraph(device, registration, solver=solver, **params) as pg:
        for p in poses:
            pg.add_node(p)
        for loop_idx, curr_idx, T, score in accepted:
            pg.add_loop(loop_idx, curr_idx, loop_measurement(poses, loop_idx, curr_idx, T, literal_measurement), score, robust_k)
        for node, xyz, var in positions or ():
            pg.add_position(node, xyz, var, robust_k)
        info = pg.optimize()
        info["weights"] = pg.weights()
        info["position_weights"] = pg.position_weights()
        info["poses"] = pg.poses()
        return pg.poses6d(), info
