"""Host-side mirror of ISCGeneration (Intensity Scan Context, pgo_node's loop_method 2) backed by libndt_hip.so
(include/ndt_hip.h, ndt_isc_*; kernels in csrc/isc.hip).

pgo_node drives the object per keyframe (xchu_mapping/src/pgo_node.cpp:222-246, 364-386):

    point = (pose.x, pose.y, 0)
    iscGeneration.makeAndSavedec(thisKeyFrame, point)
    prev, curr = iscGeneration.detectLoopClosureID()
    if prev != -1 and planar distance of the two poses <= 20 m: ICPRefine(prev, current)

`detect_loops_isc` is the offline counterpart (every keyframe of a replay tested in one launch); `close_loops(...,
loop_method=2)` chains it with that gate and `refine_loop`.  The descriptor database stays on the device.  The reference
cannot be compiled here: the semantics are the restatement in DESIGN.md §2 "ISC" (parity unpinned).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ctxobj import _CtxObject
from ._lib import IscParams, IscResult, check
from .ndt import NormalDistributionsTransform, _dp, _fp

__all__ = ["ISCGeneration", "detect_loops_isc", "color_projection"]

_PARAM_NAMES = tuple(k for k, _ in IscParams._fields_)
_RESULT_NAMES = tuple(k for k, _ in IscResult._fields_)
_UP = C.POINTER(C.c_ubyte)


def color_projection() -> np.ndarray:
    """init_color (ISCGeneration.cpp:24-49): the 272-entry RGB table in its listed order, indexed by the cell's byte
    (cv::Vec3b's constructor takes uchar: an int argument wraps modulo 256)."""
    t = [(0, i * 16, 255) for i in range(1)]
    t += [(0, i * 16, 255) for i in range(15)]
    t += [(0, 255, 255 - i * 16) for i in range(16)]
    t += [(i * 32, 255, 0) for i in range(32)]
    t += [(255, 255 - i * 16, 0) for i in range(16)]
    t += [(i * 4, 255, 0) for i in range(64)]
    t += [(255, 255 - i * 4, 0) for i in range(64)]
    t += [(255, i * 4, i * 4) for i in range(64)]
    return (np.array(t, np.int64) % 256).astype(np.uint8)


def _record(r: IscResult) -> dict:
    return {k: (float if k.endswith("_score") else int)(getattr(r, k)) for k in _RESULT_NAMES}


def _pos(pose_xyz) -> np.ndarray:
    p = np.ascontiguousarray(pose_xyz, np.float64).reshape(-1)
    if p.size != 3:
        raise ValueError("a keyframe position is (x, y, z)")
    return p


class ISCGeneration(_CtxObject):
    """ISCGeneration on MI355X.  It runs on a registration context: its own, or the one of an existing
    NormalDistributionsTransform (`registration=`), whose device and stream it then shares.  The parameters (IscParams
    fields) are fixed once the first descriptor is stored: the database layout depends on them."""

    _DESTROY = "ndt_isc_destroy"
    _WHAT = "ISC"

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None, **params):
        super().__init__(device, registration)
        self._params = self._default_params(IscParams, "ndt_isc_default_params", params)
        self._create()
        self._colors = color_projection()
        self._last = IscResult()
        self._last.loop_id = -1

    def _create(self):
        isc = C.c_void_p()
        check(self._lib.ndt_isc_create(self.ctx, C.byref(self._params), C.byref(isc)), self.ctx)
        if self._handle:
            self._lib.ndt_isc_destroy(self._handle)
        self._handle = isc

    def __len__(self) -> int:
        return int(self._lib.ndt_isc_size(self._handle))

    # ------------------------------------------------------------------ parameters
    def init_param(self, rings: int, sectors: int, max_dis: float):
        """init_param (:12-22); allowed while no descriptor is stored."""
        if len(self):
            raise RuntimeError("init_param after the first descriptor: the database layout depends on the parameters")
        new = IscParams.from_buffer_copy(self._params)
        new.rings, new.sectors, new.max_dis = int(rings), int(sectors), float(max_dis)
        old, self._params = self._params, new
        try:
            self._create()
        except Exception:
            self._params = old
            raise

    def params(self) -> dict:
        return {k: getattr(self._params, k) for k in _PARAM_NAMES}

    @property
    def shape(self) -> tuple[int, int]:
        return int(self._params.rings), int(self._params.sectors)

    # ------------------------------------------------------------------ descriptors
    def makeAndSavedec(self, cloud_xyzi, pose_xyz) -> int:
        """Descriptor of a host cloud ((N, 4) x,y,z,intensity floats) taken at position pose_xyz (pgo_node passes
        z = 0); returns its index."""
        a = np.ascontiguousarray(cloud_xyzi, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 4:
            raise ValueError("expected (N, 4) x,y,z,intensity")
        idx = C.c_int()
        check(self._lib.ndt_isc_add(self._handle, _fp(a), a.shape[0], a.shape[1] * 4, 3, _dp(_pos(pose_xyz)), C.byref(idx)), self.ctx)
        return idx.value

    def makeAndSavedecDevice(self, d_ptr: int, n: int, pose_xyz) -> int:
        """The same of a device-resident float4 x,y,z,intensity cloud (no transfer); it stays unmodified until the next
        detection."""
        idx = C.c_int()
        check(self._lib.ndt_isc_add_device(self._handle, C.c_void_p(d_ptr), int(n), _dp(_pos(pose_xyz)), C.byref(idx)), self.ctx)
        return idx.value

    def add_descriptor(self, desc, pose_xyz) -> int:
        """A ready rings x sectors byte matrix."""
        d = np.ascontiguousarray(desc, np.uint8)
        if d.shape != self.shape:
            raise ValueError(f"a descriptor is {self.shape[0]} x {self.shape[1]}")
        idx = C.c_int()
        check(self._lib.ndt_isc_add_descriptor(self._handle, d.ctypes.data_as(_UP), _dp(_pos(pose_xyz)), C.byref(idx)), self.ctx)
        return idx.value

    def descriptor(self, i: int) -> np.ndarray:
        d = np.empty(self.shape, np.uint8)
        check(self._lib.ndt_isc_get(self._handle, int(i), d.ctypes.data_as(_UP), None, None), self.ctx)
        return d

    def position(self, i: int) -> tuple[np.ndarray, float]:
        """(position as stored, travel distance) of keyframe i."""
        p, t = np.empty(3, np.float64), C.c_double()
        check(self._lib.ndt_isc_get(self._handle, int(i), None, _dp(p), C.byref(t)), self.ctx)
        return p, t.value

    def getLastISCMONO(self) -> np.ndarray:
        return self.descriptor(len(self) - 1)

    def getLastISCRGB(self) -> np.ndarray:
        """(rings, sectors, 3) uint8: the last descriptor through the colour table (:96-105)."""
        return self._colors[self.getLastISCMONO()]

    # ------------------------------------------------------------------ detection
    def is_loop_pair(self, i: int, j: int) -> tuple[bool, float, float]:
        """(is_loop, geo_score, inten_score) of stored descriptors i and j; inten_score is computed whatever the
        geometry score is."""
        geo, inten, angle, loop = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        check(self._lib.ndt_isc_pair(self._handle, int(i), int(j), C.byref(geo), C.byref(angle), C.byref(inten), C.byref(loop)), self.ctx)
        return bool(loop.value), geo.value, inten.value

    def calculate_geometry_dis(self, i: int, j: int) -> tuple[float, int]:
        geo, angle = C.c_double(), C.c_int()
        check(self._lib.ndt_isc_pair(self._handle, int(i), int(j), C.byref(geo), C.byref(angle), None, None), self.ctx)
        return geo.value, angle.value

    def calculate_intensity_dis(self, i: int, j: int, angle: int) -> float:
        inten = C.c_double()
        check(self._lib.ndt_isc_intensity(self._handle, int(i), int(j), int(angle), C.byref(inten)), self.ctx)
        return inten.value

    def detectLoopClosureID(self) -> tuple[int, float]:
        """(prev, float(curr)) or (-1, 0.0), the reference's std::pair<int, float>."""
        check(self._lib.ndt_isc_detect(self._handle, C.byref(self._last)), self.ctx)
        if self._last.loop_id == -1:
            return -1, 0.0
        return int(self._last.loop_id), float(np.float32(self._last.curr_id))

    def last_result(self) -> dict:
        """The whole record of the last detectLoopClosureID."""
        return _record(self._last)

    def detect_batch(self, query) -> list[dict]:
        """Stateless: every query[k] tested as if it were the newest keyframe, all in one launch."""
        q = np.ascontiguousarray(query, np.int32)
        if q.ndim != 1:
            raise ValueError("query is 1-D")
        out = (IscResult * max(1, len(q)))()
        check(self._lib.ndt_isc_detect_batch(self._handle, q.ctypes.data_as(C.POINTER(C.c_int)), len(q), out), self.ctx)
        return [_record(out[i]) for i in range(len(q))]


def detect_loops_isc(keyframes=None, poses=None, device: int = 0, registration=None, descriptors=None, **params) -> list[dict]:
    """Every keyframe of a replay tested for a loop in one launch (the offline counterpart of calling detectLoopClosureID
    after each makeAndSavedec).  keyframes: (N, 4) x,y,z,intensity clouds, or `descriptors`: ready byte matrices; poses:
    per keyframe (x, y, ...) — the position handed over is (x, y, 0), as pgo_node does.  **params are IscParams fields.
    One record per keyframe, as ISCGeneration.last_result."""
    if (keyframes is None) == (descriptors is None):
        raise ValueError("give either keyframes or descriptors")
    items = keyframes if descriptors is None else descriptors
    if poses is None or len(poses) != len(items):
        raise ValueError("poses do not match keyframes")
    with ISCGeneration(device, registration, **params) as isc:
        for k, p in zip(items, poses):
            xyz = (float(p[0]), float(p[1]), 0.0)
            if descriptors is None:
                isc.makeAndSavedec(k, xyz)
            else:
                isc.add_descriptor(k, xyz)
        return isc.detect_batch(np.arange(len(isc)))
