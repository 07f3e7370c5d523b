"""pgo_node's Run loop without ROS or GTSAM: the keyframe gate, the online back end on corrected poses, loop_method 0,
and the offline entry point that strings odom_node's front end to it (xchu_mapping/src/pgo_node.cpp:137-528).

    with xa.PGO(loop_method=1) as pgo:
        for cloud, pose, stamp in matched:        # the /filtered_points cloud and the odometry pose of one scan
            rec = pgo.push(cloud, pose, stamp)
        pgo.save(directory)

    state = xa.run_mapping(scans, stamps, directory)      # filter_scan -> LidarOdom.process -> PGO.push per scan

`keyframe_gate` is PGO::Run's movement gate (:188-205), pinned by the reference's recorded run (tests/golden/
pgo_run_1317618205: it selects the recorded keyframes exactly).  Everything after the gate is a model (DESIGN.md §2
"pgo_node loop", parity unpinned): the reference runs Run, a 2 Hz detection thread and an ICP thread concurrently, so its
order of events is not reproducible; `PGO.push` fixes one order.  Every device step is an existing launch of the store,
the detectors, refine_loop and the pose graph; this module is host code.
"""
from __future__ import annotations

import math
import time

import numpy as np

from ._ctxobj import _CtxObject
from ._lib import check
from .globalmap import KeyframeMap, save_map
from .icp import refine_loop
from .isc import ISCGeneration
from .ndt import NormalDistributionsTransform, filter_scan
from .odom import LidarOdom
from .posegraph import PoseGraph, _inv, _matrix_to_pose6d, _pose44, _poses6d, loop_measurement
from .scancontext import SCManager
from .synth import pose_matrix

__all__ = ["PGO", "keyframe_gate", "detect_loop_radius", "run_mapping"]

_START_ACCUMULATION = 1000000.0     # pgo.h:136: the first pose received is always a keyframe
_GPS_VARIANCES = (1e9, 1e9, 250.0)  # pgo_node.cpp:103-111: only the altitude is constrained
_RADIUS_ACCEPT = 30.0               # :335, loop_method 0's own distance test


class _Gate:
    """PGO::Run's keyframe rule (:188-205, pgo.h:96,136) in f64: the previous pose starts at (0, 0, 0), the accumulator at
    1 000 000; the step is taken between consecutive poses received, whether or not the earlier one became a keyframe;
    a keyframe needs accumulated > gap (strict) and resets the accumulator to 0."""

    def __init__(self, gap: float):
        self.gap = float(gap)
        self.prev = (0.0, 0.0, 0.0)
        self.moved = _START_ACCUMULATION

    def step(self, x: float, y: float, z: float) -> bool:
        px, py, pz = self.prev
        self.prev = (x, y, z)
        self.moved += math.sqrt((px - x) ** 2 + (py - y) ** 2 + (pz - z) ** 2)
        if self.moved > self.gap:
            self.moved = 0.0
            return True
        return False


def _positions(poses) -> np.ndarray:
    p = np.asarray(poses, np.float64)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        return p[:, :3, 3]
    if p.ndim == 2 and p.shape[1] >= 3:
        return p[:, :3]
    if p.size == 0:
        return np.zeros((0, 3))
    raise ValueError("poses are (N, >=3) positions / Pose6D rows or (N, 4, 4) matrices")


def keyframe_gate(poses, gap: float = 2.0) -> np.ndarray:
    """The indices of the poses PGO::Run keeps as keyframes (host numpy).  poses: (N, >=3) positions or Pose6D rows
    (x, y, z first), or (N, 4, 4) matrices, one per matched cloud/odometry pair in arrival order."""
    g = _Gate(gap)
    return np.array([k for k, (x, y, z) in enumerate(_positions(poses).tolist()) if g.step(x, y, z)], np.int64)


def detect_loop_radius(poses, times, min_keyframes: int = 30, radius: float = 20.0, min_time_gap: float = 30.0) -> int:
    """loop_method 0's candidate for the newest keyframe (PerformSCLoopClosure :300-327, host numpy): -1 below
    min_keyframes keyframes; else every stored keyframe (the newest included) whose f32 planar squared distance to the
    newest corrected pose is below radius^2 (strict), by ascending squared distance (equal distances: lower index first),
    and of those the first whose time differs from the newest's by more than min_time_gap seconds (strict); -1 when there
    is none.  poses: the corrected poses (x, y first), times: per keyframe.  The radius test's strictness and the order
    of equal distances are FLANN's, which the reference tree does not hold: modelled."""
    xy = np.asarray(poses, np.float64)[:, :2].astype(np.float32)
    t = np.asarray(times, np.float64).reshape(-1)
    n = len(xy)
    if n != len(t):
        raise ValueError("one time per keyframe pose")
    if n < min_keyframes or n == 0:
        return -1
    d = xy - xy[-1]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]               # f32, as the kd-tree's L2_Simple over pcl::PointXYZI
    near = np.flatnonzero(d2 < np.float32(radius) * np.float32(radius))
    near = near[np.argsort(d2[near], kind="stable")]
    old = near[np.abs(t[near] - t[-1]) > min_time_gap]
    return int(old[0]) if len(old) else -1


def _pose6(pose) -> np.ndarray:
    p = np.asarray(pose, np.float64)
    if p.shape == (6,):
        return p.copy()
    if p.shape == (4, 4):
        return np.array(_matrix_to_pose6d(p), np.float64)
    raise ValueError("a pose is (x, y, z, roll, pitch, yaw) or a 4 x 4 matrix")


class PGO(_CtxObject):
    """pgo_node's back end, one `push` per matched cloud/odometry pair.  It owns a KeyframeMap, the detector of its
    loop_method (1: SCManager with dist_thres 0.2; 2: ISCGeneration with init_param(60, 60, 40.0); 0: the radius rule,
    no detector) and a PoseGraph, all on one registration context: its own, or the one of an existing
    NormalDistributionsTransform (`registration=`).

    keyframe_gap: keyframeMeterGap.  leaf, search_num, score_threshold, method, literal_root: refine_loop's.
    min_keyframes: no detection below that many keyframes (:300).  max_pair_dist: the planar gate of methods 1 and 2 on
    the corrected poses (method 0 accepts below 30 m, :335).  robust_k: the Cauchy width of loop and GPS factors.
    literal_measurement: loop_measurement's.  detect_args: the detector's parameters (ScParams / IscParams fields);
    pgo_args: PoseGraph's; solver: PoseGraph's ("cg" or "direct"; a "solver" entry of pgo_args, if there is one, wins).  detect_every: detection runs on every detect_every-th keyframe.
    append: "predict" keeps the solve off keyframes that add no information (a node that brings only its odometry edge
    gets the estimate X_{k-1} (P_{k-1}^-1 P_k), no launch; while the graph holds no loop or position factor `poses` is the
    odometry bit for bit); "optimize" solves after every keyframe, the reference's sequence of ISAM2Update calls.
    literal_reject_stops: the reference's ICP thread returns on its first rejected loop (:443-445) and refines nothing
    afterwards; True reproduces that."""

    _WHAT = "pgo_node"
    _store = _detector = _graph = None

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None, loop_method: int = 1,
                 keyframe_gap: float = 2.0, leaf: float = 0.5, min_keyframes: int = 30, max_pair_dist: float = 20.0,
                 search_num: int = 25, score_threshold: float = 0.3, method: str = "icp", robust_k: float = 1.0,
                 literal_measurement: bool = False, literal_root: bool = False, detect_args: dict | None = None,
                 pgo_args: dict | None = None, append: str = "predict", detect_every: int = 1,
                 literal_reject_stops: bool = False, solver="cg"):
        if loop_method not in (0, 1, 2):
            raise ValueError("loop_method is 0 (radius search), 1 (Scan Context) or 2 (Intensity Scan Context)")
        if append not in ("predict", "optimize"):
            raise ValueError("append must be 'predict' or 'optimize'")
        if detect_every < 1:
            raise ValueError("detect_every is at least 1")
        if loop_method == 0 and detect_args:
            raise ValueError("loop_method 0 has no detector to configure")
        super().__init__(device, registration)
        self.loop_method, self.append, self.detect_every = loop_method, append, int(detect_every)
        self.min_keyframes, self.max_pair_dist, self.robust_k = int(min_keyframes), float(max_pair_dist), float(robust_k)
        self.literal_measurement, self.literal_reject_stops = bool(literal_measurement), bool(literal_reject_stops)
        self._refine = dict(search_num=search_num, leaf=leaf, score_threshold=score_threshold, method=method,
                            literal_root=literal_root)
        self.leaf = float(leaf)
        self.sync_timings = False   # True: wait for the stream after each stage, so that rec["ms"] splits device time
        self.keep_poses_before = True   # False: the log keeps poses_before only for refined records (push still returns it)
        self._store = self._detector = self._graph = None
        try:
            self._store = KeyframeMap(registration=self._reg)
            args = {k: v for k, v in (detect_args or {}).items() if k != "device"}
            if loop_method == 1:
                self._detector = SCManager(registration=self._reg, **dict({"dist_thres": 0.2}, **args))
            elif loop_method == 2:
                self._detector = ISCGeneration(registration=self._reg, **dict({"rings": 60, "sectors": 60, "max_dis": 40.0}, **args))
            self._graph = PoseGraph(registration=self._reg, **dict({"solver": solver}, **(pgo_args or {})))
        except Exception:
            self.close()
            raise
        self._gate = _Gate(keyframe_gap)
        self._odom: list[np.ndarray] = []
        self._times: list[float] = []
        self._P = np.empty((64, 6))         # poses: rows [:n] of a buffer that is replaced, never rewritten, on an optimise
        self._X_last = None                 # the estimate of the newest node once the graph holds more than odometry
        self._informative = False           # a loop or position factor is in the graph
        self._gps_offset = None
        self._stopped = False               # literal_reject_stops: a loop was rejected
        self.scans = 0
        self.optimize_launches = 0
        self.cg_iterations = 0
        self._loops, self._rejected, self._log = [], [], []

    def close(self):
        for obj in (self._detector, self._graph, self._store):   # before their context
            if obj is not None:
                obj.close()
        self._detector = self._graph = self._store = None
        super().close()

    # ------------------------------------------------------------------ state
    def __len__(self) -> int:
        return len(self._odom)

    @property
    def odom_poses(self) -> np.ndarray:
        """keyframePoses: the odometry pose of every keyframe as given, (n, 6)."""
        return np.array(self._odom, np.float64).reshape(len(self._odom), 6)

    @property
    def poses(self) -> np.ndarray:
        """keyframePosesUpdated: the corrected pose of every keyframe, (n, 6), read-only."""
        v = self._P[:len(self._odom)]
        v.setflags(write=False)
        return v

    @property
    def times(self) -> np.ndarray:
        return np.array(self._times, np.float64)

    @property
    def loops(self) -> list:
        """Accepted loops, [(loop_idx, curr_idx, transform, score)] as close_loops returns them."""
        return list(self._loops)

    @property
    def rejected(self) -> list:
        """[(loop_idx, curr_idx, reason)], reason "pair_distance" or "icp"."""
        return list(self._rejected)

    @property
    def store(self) -> KeyframeMap:
        return self._store

    @property
    def detector(self):
        return self._detector

    @property
    def graph(self) -> PoseGraph:
        return self._graph

    @property
    def log(self) -> list:
        """The record of every keyframe, as push returned it.  A record's poses_before is a view of a buffer that every
        optimise replaces, so under append="optimize" the log grows by a pose array per keyframe (O(n^2) doubles, 114 MB
        at 1541 keyframes); with keep_poses_before = False the log drops the field from records that were not refined."""
        return self._log

    # ------------------------------------------------------------------ Run
    def _sync(self):
        if self.sync_timings:
            check(self._lib.ndt_synchronize(self.ctx), self.ctx)

    def _append_row(self, row):
        n = len(self._odom) - 1            # the new keyframe's index
        if n >= len(self._P):
            grown = np.empty((2 * len(self._P), 6))
            grown[:n] = self._P[:n]
            self._P = grown
        self._P[n] = row

    def _optimize(self) -> dict:
        info = self._graph.optimize()
        self.optimize_launches += 1
        self.cg_iterations += info["cg_iterations"]
        T = self._graph.poses()
        P = np.empty((max(len(self._P), len(T)), 6))
        P[:len(T)] = _poses6d(T)
        self._P, self._X_last = P, T[-1]
        return info

    def push(self, cloud, odom_pose, stamp: float, gps_altitude: float | None = None) -> dict:
        """One call of PGO::Run for a matched pair: cloud (N, 4) x,y,z,intensity in the sensor frame, odom_pose (x, y, z,
        roll, pitch, yaw) or 4 x 4, stamp in seconds, gps_altitude the altitude of the fix matched to this scan (useGPS) or
        None.  Returns {"keyframe": False} for a scan the gate drops (nothing touches the device), else the keyframe's
        record: index, candidate (loop index or -1), gate ("ok", "pair_distance", "too_few", "none"), refined, accepted,
        score, transform, measurement (the loop factor's Z), poses_before (the corrected poses that moved the submaps and
        that the gate and the measurement used), optimized, info (optimize()'s dict or None), gps (the position factor's
        xyz or None) and ms (wall milliseconds of store, detect, refine, optimize)."""
        # everything that can be refused is looked at before any state moves: the gate, the store, the detector and the
        # graph must stay in step
        p6 = _pose6(odom_pose)
        if not np.all(np.isfinite(p6)):
            raise ValueError("the odometry pose is not finite")
        a = np.ascontiguousarray(cloud, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("a keyframe is an (N, 4) x,y,z,intensity array")
        stamp = float(stamp)
        if gps_altitude is not None and not math.isfinite(float(gps_altitude)):
            raise ValueError("the GPS altitude is not finite")
        P_k = _pose44(p6)
        self.scans += 1
        if not self._gate.step(float(p6[0]), float(p6[1]), float(p6[2])):
            return {"keyframe": False}
        if gps_altitude is not None and self._gps_offset is None:
            self._gps_offset = float(gps_altitude)         # :207-212: the first keyframe that has a fix
        ms = dict.fromkeys(("store", "detect", "refine", "optimize"), 0.0)
        t0 = time.perf_counter()
        # the store (one upload) and the descriptor from the store's device pointer
        k = self._store.add(a)
        if self._detector is not None:
            ptr, n_pts = self._store.keyframe_device(k)
            if self.loop_method == 1:
                self._detector.makeAndSaveScancontextAndKeysDevice(ptr, n_pts)
            else:
                self._detector.makeAndSavedecDevice(ptr, n_pts, (p6[0], p6[1], 0.0))     # :222-239
        self._sync()
        ms["store"] = 1e3 * (time.perf_counter() - t0)
        # the graph node with its prior or odometry edge, the position factor, and the estimate
        t0 = time.perf_counter()
        P_prev = _pose44(self._odom[-1]) if self._odom else None
        self._odom.append(p6)
        self._times.append(stamp)
        self._graph.add_node(P_k)
        gps = None
        if gps_altitude is not None and k > 0:             # :278-287: x, y of the last optimised pose, the altitude offset
            gps = np.array([self._P[k - 1, 0], self._P[k - 1, 1], float(gps_altitude) - self._gps_offset])
            self._graph.add_position(k, gps, _GPS_VARIANCES, self.robust_k)
            self._informative = True
        info = None
        if self.append == "optimize" or gps is not None:
            self._append_row(p6)
            info = self._optimize()
        elif not self._informative:
            self._append_row(p6)                           # prior and odometry edges alone: the input is the optimum
        else:
            X_k = self._X_last @ (_inv(P_prev) @ P_k)      # the new edge's residual is zero: stationary stays stationary
            self._graph.set_estimate(k, X_k)
            self._append_row(_poses6d(X_k[None])[0])
            self._X_last = X_k
        ms["optimize"] = 1e3 * (time.perf_counter() - t0)
        rec = {"keyframe": True, "index": k, "candidate": -1, "gate": "none", "refined": False, "accepted": False, "score": None,
               "transform": None, "measurement": None, "poses_before": self.poses, "optimized": info is not None, "info": info,
               "gps": gps, "ms": ms}
        self._close(rec, k, ms)
        if self.keep_poses_before or rec["refined"]:
            self._log.append(rec)
        else:
            self._log.append(dict(rec, poses_before=None))
        return rec

    def _close(self, rec: dict, k: int, ms: dict):
        """Steps 5 to 8 of push for keyframe k: detection, the gate, the refinement and the loop factor; fills rec."""
        n = k + 1
        if n < self.min_keyframes:
            rec["gate"] = "too_few"
            return rec
        if k % self.detect_every:
            return rec
        t0 = time.perf_counter()
        before = rec["poses_before"]
        if self.loop_method == 0:
            cand = detect_loop_radius(before, self._times, self.min_keyframes)
        else:
            cand = int(self._detector.detectLoopClosureID()[0])
        ms["detect"] = 1e3 * (time.perf_counter() - t0)
        rec["candidate"] = cand
        if cand == -1:
            return rec
        # the planar gate on the corrected poses
        dist = math.sqrt((before[cand, 0] - before[k, 0]) ** 2 + (before[cand, 1] - before[k, 1]) ** 2)
        if (not dist < _RADIUS_ACCEPT) if self.loop_method == 0 else dist > self.max_pair_dist:
            rec["gate"] = "pair_distance"
            self._rejected.append((cand, k, "pair_distance"))
            return rec
        rec["gate"] = "ok"
        if self._stopped:
            return rec
        # ICPRefine on the corrected poses
        t0 = time.perf_counter()
        out = refine_loop(None, before, cand, k, store=self._store, **self._refine)
        ms["refine"] = 1e3 * (time.perf_counter() - t0)
        rec.update(refined=True, accepted=out["accepted"], score=out["score"], transform=out["transform"])
        if not out["accepted"]:
            self._rejected.append((cand, k, "icp"))
            self._stopped = self.literal_reject_stops
            return rec
        t0 = time.perf_counter()
        # :465-466: the f32 ICP result goes through Matrix2Pose6D and Pose6D2Pose3, which makes it a rotation again
        T_icp = pose_matrix(*_matrix_to_pose6d(np.asarray(out["transform"], np.float64)))
        Z = loop_measurement(before, cand, k, T_icp, self.literal_measurement)
        self._graph.add_loop(cand, k, Z, out["score"], self.robust_k)
        self._informative = True
        self._loops.append((cand, k, out["transform"], out["score"]))
        info = self._optimize()
        ms["optimize"] += 1e3 * (time.perf_counter() - t0)
        rec.update(measurement=Z, optimized=True, info=info)
        return rec

    def save(self, directory, odom=None) -> np.ndarray:
        """PGO::SaveMap with the corrected poses: save_map(directory, store, poses, times, odom); returns the final map."""
        return save_map(directory, self._store, self.poses, self.times, odom, self.leaf)


def run_mapping(scans, stamps, directory=None, odom_args: dict | None = None, filter_args: dict | None = None, **pgo_args) -> dict:
    """The three nodes offline (the reference README's "offline version"): each scan ((N, 4) x,y,z,intensity) goes
    through filter_scan (filter_node), LidarOdom.process (odom_node) and PGO.push (pgo_node) with the filtered cloud and
    the odometry's current_pose; with a directory, SaveMap's files are written at the end (lidar_odom.txt included).
    odom_args: LidarOdom's parameters; filter_args: filter_scan's; **pgo_args: PGO's (solver= among them).

    Returns the back end's state and the per-scan odometry: keyframes (the scan index of every keyframe), odom_poses,
    poses, times, loops, rejected, log, odometry ((N, 6) current_pose per scan), stamps, optimize_launches,
    cg_iterations and final_map (None without a directory)."""
    stamps = np.asarray(stamps, np.float64).reshape(-1)
    if len(stamps) != len(scans):
        raise ValueError("one stamp per scan")
    device = pgo_args.get("device", 0)
    fargs = {k: v for k, v in (filter_args or {}).items() if k not in ("device", "ndt", "stats")}
    odom = LidarOdom(device=device, **(odom_args or {}))
    try:
        with PGO(**pgo_args) as pgo:
            odometry, keyframes = np.empty((len(scans), 6)), []
            for i, (scan, stamp) in enumerate(zip(scans, stamps)):
                cloud = filter_scan(scan, ndt=pgo.registration, **fargs)
                odometry[i] = odom.process(cloud, float(stamp))["current_pose"]
                if pgo.push(cloud, odometry[i], float(stamp))["keyframe"]:
                    keyframes.append(i)
            final = pgo.save(directory, (stamps, odometry)) if directory is not None else None
            return {"keyframes": np.array(keyframes, np.int64), "odom_poses": pgo.odom_poses, "poses": pgo.poses.copy(),
                    "times": pgo.times, "loops": pgo.loops, "rejected": pgo.rejected, "log": pgo.log, "odometry": odometry,
                    "stamps": stamps, "optimize_launches": pgo.optimize_launches, "cg_iterations": pgo.cg_iterations,
                    "final_map": final}
    finally:
        odom.close()
