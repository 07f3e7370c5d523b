"""Host-side mirror of SCManager (Scan Context, pgo_node's default loop detector) backed by libndt_hip.so
(include/ndt_hip.h, ndt_sc_*; kernels in csrc/scancontext.hip).

pgo_node drives the object per keyframe (/root/reference/xchu_mapping/src/pgo_node.cpp:236, 344-362):

    scManager.makeAndSaveScancontextAndKeys(*thisKeyFrame)
    loop_id, yaw_diff = scManager.detectLoopClosureID()
    if loop_id != -1 and planar distance of the two poses <= 20 m: ICPRefine(loop_id, current)

`detect_loops` is the offline counterpart (every keyframe of a replay tested in one launch) and `close_loops` chains it
with that gate and `refine_loop`, without ROS or GTSAM.  The descriptor database stays on the device.  The reference
cannot be compiled here: the semantics are the restatement in DESIGN.md (parity unpinned).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._ctxobj import _CtxObject
from ._lib import ScParams, ScResult, check
from .globalmap import KeyframeMap
from .icp import refine_loop
from .isc import detect_loops_isc
from .ndt import NormalDistributionsTransform, _dp, _fp, as_points

__all__ = ["SCManager", "detect_loops", "close_loops", "search_schedule"]

N_RING, N_SECTOR = 20, 60
_PARAM_NAMES = tuple(k for k, _ in ScParams._fields_)


def _record(r: ScResult) -> dict:
    n = int(r.n_candidates)
    return {"loop_id": int(r.loop_id), "yaw_diff": np.float32(r.yaw_diff), "min_dist": float(r.min_dist), "nn_idx": int(r.nn_idx),
            "nn_align": int(r.nn_align), "cand_idx": [int(v) for v in r.cand_idx[:n]], "cand_dist": [float(v) for v in r.cand_dist[:n]],
            "cand_shift": [int(v) for v in r.cand_shift[:n]]}


class SCManager(_CtxObject):
    """SCManager on MI355X.  It runs on a registration context: its own, or the one of an existing
    NormalDistributionsTransform (`registration=`), whose device and stream it then shares."""

    _DESTROY = "ndt_sc_destroy"
    _WHAT = "Scan Context"

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None, **params):
        super().__init__(device, registration)
        self._params = self._default_params(ScParams, "ndt_sc_default_params", params)
        sc = C.c_void_p()
        check(self._lib.ndt_sc_create(self.ctx, C.byref(self._params), C.byref(sc)), self.ctx)
        self._handle = sc
        self._last = ScResult()
        self._last.loop_id = -1

    def __len__(self) -> int:
        return int(self._lib.ndt_sc_size(self._handle))

    # ------------------------------------------------------------------ parameters
    def set_params(self, **params):
        new = self._with_overrides(ScParams.from_buffer_copy(self._params), params)
        check(self._lib.ndt_sc_set_params(self._handle, C.byref(new)), self.ctx)
        self._params = new

    def params(self) -> dict:
        return {k: getattr(self._params, k) for k in _PARAM_NAMES}

    def setSCdistThres(self, thres: float):
        self.set_params(dist_thres=float(thres))

    # ------------------------------------------------------------------ descriptors
    def makeAndSaveScancontextAndKeys(self, cloud) -> int:
        """Descriptor, ring key and sector key of a host cloud ((N, >=3) floats or PointXYZI records); returns its index."""
        buf, stride = as_points(cloud)
        idx = C.c_int()
        check(self._lib.ndt_sc_add(self._handle, _fp(buf), len(buf) if buf.ndim == 2 else buf.size * 4 // stride, stride, C.byref(idx)), self.ctx)
        return idx.value

    def makeAndSaveScancontextAndKeysDevice(self, d_ptr: int, n: int) -> int:
        """The same of a device-resident float4 cloud (no transfer); it stays unmodified until the next detection."""
        idx = C.c_int()
        check(self._lib.ndt_sc_add_device(self._handle, C.c_void_p(d_ptr), int(n), C.byref(idx)), self.ctx)
        return idx.value

    def saveScancontextAndKeys(self, desc) -> int:
        d = np.asarray(desc, np.float64)
        if d.shape != (N_RING, N_SECTOR):
            raise ValueError("a descriptor is 20 x 60")
        colmajor = np.ascontiguousarray(d.T).reshape(-1)
        idx = C.c_int()
        check(self._lib.ndt_sc_add_descriptor(self._handle, _dp(colmajor), C.byref(idx)), self.ctx)
        return idx.value

    def _get(self, i: int):
        desc = np.empty(N_RING * N_SECTOR, np.float64)
        rk = np.empty(N_RING, np.float32)
        sk = np.empty(N_SECTOR, np.float64)
        check(self._lib.ndt_sc_get(self._handle, int(i), _dp(desc), _fp(rk), _dp(sk)), self.ctx)
        return desc.reshape(N_SECTOR, N_RING).T.copy(), rk, sk

    def polarcontext(self, i: int) -> np.ndarray:
        return self._get(i)[0]

    def ringkey(self, i: int) -> np.ndarray:
        return self._get(i)[1]

    def sectorkey(self, i: int) -> np.ndarray:
        return self._get(i)[2]

    def getConstRefRecentSCD(self) -> np.ndarray:
        return self.polarcontext(len(self) - 1)

    # ------------------------------------------------------------------ detection
    def distanceBtnScanContext(self, i: int, j: int) -> tuple[float, int]:
        dist, shift = C.c_double(), C.c_int()
        check(self._lib.ndt_sc_distance(self._handle, int(i), int(j), C.byref(dist), C.byref(shift)), self.ctx)
        return dist.value, shift.value

    def detectLoopClosureID(self) -> tuple[int, np.float32]:
        check(self._lib.ndt_sc_detect(self._handle, C.byref(self._last)), self.ctx)
        return int(self._last.loop_id), np.float32(self._last.yaw_diff)

    def last_result(self) -> dict:
        """The whole record of the last detectLoopClosureID: candidates, their distances and shifts, the best one."""
        return _record(self._last)

    def detect_batch(self, query, n_search) -> list[dict]:
        """Stateless: query[i] against the ring keys [0, n_search[i]), all in one launch."""
        q = np.ascontiguousarray(query, np.int32)
        ns = np.ascontiguousarray(n_search, np.int32)
        if q.shape != ns.shape or q.ndim != 1:
            raise ValueError("query and n_search are 1-D and of equal length")
        out = (ScResult * max(1, len(q)))()
        ip = C.POINTER(C.c_int)
        check(self._lib.ndt_sc_detect_batch(self._handle, q.ctypes.data_as(ip), ns.ctypes.data_as(ip), len(q), out), self.ctx)
        return [_record(out[i]) for i in range(len(q))]


def search_schedule(n: int, tree_making_period: int = 30, num_exclude_recent: int = 30) -> list[int]:
    """The searchable ring-key prefix of each of n keyframes when detectLoopClosureID runs once after every add: rebuilt
    to size - num_exclude_recent whenever the period counter is a multiple of the period (the early return below
    num_exclude_recent + 1 descriptors leaves the counter alone), stale in between."""
    out, counter, searchable = [], 0, 0
    for q in range(n):
        size = q + 1
        if size < num_exclude_recent + 1:
            out.append(0)
            continue
        if counter % tree_making_period == 0:
            searchable = size - num_exclude_recent
        counter += 1
        out.append(searchable)
    return out


def detect_loops(keyframes=None, tree_making_period: int = 1, device: int = 0, registration=None, descriptors=None,
                 **params) -> list[dict]:
    """Every keyframe of a replay tested for a loop in one launch (the offline counterpart of calling
    detectLoopClosureID after each makeAndSaveScancontextAndKeys).  Give either `keyframes`, host clouds ((N, >=3) floats
    or PointXYZI records) whose descriptors are built on the device, or `descriptors`, ready 20 x 60 arrays
    (saveScancontextAndKeys).  **params are the detector's settings (ScParams fields: dist_thres, num_exclude_recent,
    num_candidates, search_ratio).  One record per keyframe, as SCManager.last_result."""
    if (keyframes is None) == (descriptors is None):
        raise ValueError("give either keyframes or descriptors")
    with SCManager(device, registration, tree_making_period=tree_making_period, **params) as sc:
        if descriptors is not None:
            for d in descriptors:
                sc.saveScancontextAndKeys(d)
        else:
            for k in keyframes:
                sc.makeAndSaveScancontextAndKeys(k)
        n = len(sc)
        sched = search_schedule(n, tree_making_period, sc.params()["num_exclude_recent"])
        return sc.detect_batch(np.arange(n), sched)


def close_loops(keyframes, poses, max_pair_dist: float = 20.0, detect_args: dict | None = None, loop_method: int = 1,
                store=None, **refine_args):
    """pgo_node's loop-closure path for a whole replay: detect_loops, PerformSCLoopClosure's gate (pgo_node.cpp:351-362:
    the planar distance between the two keyframe poses must not exceed 20 m), then refine_loop (PGO::ICPRefine) for each
    surviving pair.  keyframes: (N, 4) x,y,z,intensity clouds; poses: per keyframe (x, y, z, roll, pitch, yaw).

    loop_method is pgo_node's switch: 1 (default) detects with Scan Context, 2 with Intensity Scan Context
    (detect_loops_isc, which reads the keyframes' fourth column; the same gate follows, pgo_node.cpp:373-384), and
    detect_args then holds detect_loops_isc's keywords (device and IscParams fields).

    Two sets of settings go in, kept apart because both callees take keyword settings of their own:
    detect_args: a dict handed to detect_loops as keywords — tree_making_period, device, and the detector's dist_thres,
        num_exclude_recent, num_candidates, search_ratio (None: the reference's constants, period 1);
    **refine_args: every other keyword goes to refine_loop unchanged — search_num, leaf, score_threshold, device,
        resolution, literal_root.

    store: a KeyframeMap holding the keyframes on the device, or True to build one from `keyframes` once for this call
    (on refine_args' device): every refine_loop then builds its submaps from the resident keyframes instead of uploading
    them again per loop, with the same results.  With a KeyframeMap given, `keyframes` may be None: the detector then
    reads the clouds back from the store.

    Returns (accepted, rejected): accepted = [(loop_idx, curr_idx, transform, score)], rejected =
    [(loop_idx, curr_idx, reason)] with reason "pair_distance" or "icp"."""
    if store is True:
        with KeyframeMap(refine_args.get("device", 0)) as built:
            for k in keyframes:
                built.add(k)
            return close_loops(keyframes, poses, max_pair_dist, detect_args, loop_method, built, **refine_args)
    if store is not None and keyframes is None:
        keyframes = [store.keyframe(i) for i in range(len(store))]
    if len(poses) != len(keyframes):
        raise ValueError("poses do not match keyframes")
    if store is not None:
        if len(store) != len(keyframes):
            raise ValueError("the store does not match keyframes")
        refine_args = dict(refine_args, store=store)
    if loop_method == 1:
        records = detect_loops([np.asarray(k)[:, :3] for k in keyframes], **(detect_args or {}))
    elif loop_method == 2:
        records = detect_loops_isc(keyframes, poses, **(detect_args or {}))
    else:
        raise ValueError("loop_method is 1 (Scan Context) or 2 (Intensity Scan Context)")
    accepted, rejected = [], []
    for curr, rec in enumerate(records):
        prev = rec["loop_id"]
        if prev == -1:
            continue
        dist = math.sqrt((poses[prev][0] - poses[curr][0]) ** 2 + (poses[prev][1] - poses[curr][1]) ** 2)
        if dist > max_pair_dist:
            rejected.append((prev, curr, "pair_distance"))
            continue
        out = refine_loop(keyframes, poses, prev, curr, **refine_args)
        if out["accepted"]:
            accepted.append((prev, curr, out["transform"], out["score"]))
        else:
            rejected.append((prev, curr, "icp"))
    return accepted, rejected
