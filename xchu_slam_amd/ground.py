"""filter_node's ground detection on MI355X, backed by libndt_hip.so (include/ndt_hip.h, ndt_ground_*; kernels in
csrc/ground.hip).

The reference's CloudFilter (xchu_mapping/src/filter_node.cpp) does two things per scan: `Run` filters the scan into
/filtered_points (`filter_scan`), and `DetectPlane` finds the floor in it: tilt, height clip, normal filter, RANSAC plane,
the gates on the inlier count and the floor's normal.  It publishes the coefficients on /ground_coeffs and the clouds
/normal_ground_points, /ground_points and /no_ground_points.

    floor = xa.detect_ground(filtered_points)          # DetectPlane
    floor.coeffs, floor.reason, floor.ground(), floor.no_ground(), floor.normal_ground()
    cf = xa.CloudFilter(); filtered, floor = cf.run(scan)   # the node's whole Run

PCL is not available to compare against: the semantics are the restatement in DESIGN.md §2 "Ground" (parity unpinned).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._ctxobj import _CtxObject
from ._lib import FilterParams, GroundParams, check
from ._lib import GroundResult as _GroundRecord
from .ndt import NormalDistributionsTransform, _fp

__all__ = ["detect_ground", "CloudFilter", "GroundResult", "GROUND_REASONS"]

GROUND_REASONS = ("OK", "TOO_FEW_POINTS", "TOO_FEW_INLIERS", "NOT_VERTICAL")
_IP = C.POINTER(C.c_int)


def ground_params(lib, **overrides) -> GroundParams:
    """The reference's values (ndt_ground_default_params) with the keyword overrides set."""
    p = GroundParams()
    p.struct_size = C.sizeof(GroundParams)
    check(lib.ndt_ground_default_params(C.byref(p)))
    names = tuple(k for k, _ in GroundParams._fields_ if k != "struct_size")
    for k, v in overrides.items():
        if k not in names:
            raise TypeError(f"unknown ground parameter {k!r}")
        setattr(p, k, v)
    return p


def _record() -> _GroundRecord:
    r = _GroundRecord()
    r.struct_size = C.sizeof(_GroundRecord)
    return r


class GroundResult:
    """One scan's floor.  `coeffs` is (a, b, c, d) with the normal upward, or None when no floor was found (`reason`
    says why; the reference returns Vector4f::Identity() there).  The clouds are read from the context the detect ran
    on, so they are those of its last detect."""

    def __init__(self, reg: NormalDistributionsTransform, rec: _GroundRecord):
        self._reg = reg
        self._clouds: dict[int, np.ndarray] = {}
        self.found = bool(rec.found)
        self.coeffs = np.array(rec.coeffs, np.float32) if rec.found else None
        self.reason = GROUND_REASONS[rec.reason]
        self.n_input, self.n_clipped, self.n_normal, self.n_inliers = rec.n_input, rec.n_clipped, rec.n_normal, rec.n_inliers
        self.iterations, self.skipped, self.k = rec.iterations, rec.skipped, float(rec.k)
        self.winner = tuple(rec.winner) if rec.winner[0] >= 0 else None
        self.stream_fallbacks = rec.stream_fallbacks

    def _cloud(self, which: int) -> np.ndarray:
        if which not in self._clouds:
            reg = self._reg
            out = np.empty((max(1, self.n_input), 4), np.float32)
            n = C.c_size_t()
            st = reg._lib.ndt_ground_cloud(reg.ctx, which, _fp(out), self.n_input, C.byref(n))
            if st not in (_lib.NDT_OK, _lib.NDT_EOVERFLOW):
                check(st, reg.ctx)
            self._clouds[which] = out[: n.value].copy()
        return self._clouds[which]

    def normal_ground(self) -> np.ndarray:
        """/normal_ground_points: the cloud after the height clip and the normal filter, (K, 4)."""
        return self._cloud(_lib.GROUND_CLOUD_NORMAL)

    def ground(self) -> np.ndarray:
        """/ground_points: the floor's inliers, (K, 4); empty when no floor was found."""
        return self._cloud(_lib.GROUND_CLOUD_GROUND)

    def no_ground(self) -> np.ndarray:
        """/no_ground_points: the input cloud without the ground, (K, 4); empty when no floor was found."""
        return self._cloud(_lib.GROUND_CLOUD_NO_GROUND)

    def _take_all(self):
        for which in (_lib.GROUND_CLOUD_NORMAL, _lib.GROUND_CLOUD_GROUND, _lib.GROUND_CLOUD_NO_GROUND):
            self._cloud(which)
        self._reg = None


def _as_cloud(cloud) -> np.ndarray:
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 4:
        raise ValueError("expected (N, 4) x,y,z,intensity")
    return a


def detect_ground(cloud, ndt: NormalDistributionsTransform | None = None, device: int = 0, **params) -> GroundResult:
    """CloudFilter::DetectPlane over an (N, 4) cloud.  `params`: the fields of ndt_ground_params (filter_node's
    tilt_deg, sensor_height, height_clip_range, floor_pts_thresh, floor_normal_thresh, use_normal_filtering,
    normal_filter_thresh; normal_k, ransac_threshold, ransac_probability, ransac_max_iterations; literal_no_ground,
    cloud_leaf).  With `ndt` the detect runs on that context and the clouds are read from it on request; without,
    on a context of its own, and the three clouds are taken before it is closed."""
    a = _as_cloud(cloud)
    own = ndt is None
    if own:
        ndt = NormalDistributionsTransform(device)
    try:
        prm = ground_params(ndt._lib, **params)
        rec = _record()
        check(ndt._lib.ndt_ground_detect(ndt.ctx, C.byref(prm), _fp(a), a.shape[0], a.shape[1] * 4, 3, C.byref(rec)), ndt.ctx)
        res = GroundResult(ndt, rec)
        if own:
            res._take_all()
        return res
    finally:
        if own:
            ndt.close()


class CloudFilter(_CtxObject):
    """filter_node's CloudFilter: `run(scan)` is the node's Run, the scan filter followed by DetectPlane over its output
    (ndt_filter_ground_scan: the filtered cloud stays on the device in between).  Keyword parameters are filter_node's
    (the fields of ndt_filter_params and ndt_ground_params)."""

    _WHAT = "CloudFilter"

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None, **params):
        super().__init__(device, registration)
        fnames = tuple(k for k, _ in FilterParams._fields_)
        self._fprm = self._default_params(FilterParams, "ndt_filter_default_params", {k: v for k, v in params.items() if k in fnames})
        self._gprm = ground_params(self._lib, **{k: v for k, v in params.items() if k not in fnames})

    def set_params(self, **params):
        """Changes filter_node parameters (the fields of ndt_filter_params and ndt_ground_params) for the next scans."""
        fnames = tuple(k for k, _ in FilterParams._fields_)
        self._with_overrides(self._fprm, {k: v for k, v in params.items() if k in fnames})
        gnames = tuple(k for k, _ in GroundParams._fields_ if k != "struct_size")
        for k, v in params.items():
            if k in fnames:
                continue
            if k not in gnames:
                raise TypeError(f"unknown {self._WHAT} parameter {k!r}")
            setattr(self._gprm, k, v)

    def detect_plane(self, cloud) -> GroundResult:
        """DetectPlane over an already filtered cloud."""
        a = _as_cloud(cloud)
        rec = _record()
        check(self._lib.ndt_ground_detect(self.ctx, C.byref(self._gprm), _fp(a), a.shape[0], a.shape[1] * 4, 3, C.byref(rec)), self.ctx)
        return GroundResult(self._reg, rec)

    def run(self, scan):
        """Returns (filtered_points (K, 4), floor)."""
        a = _as_cloud(scan)
        n = a.shape[0]
        lib, ctx = self._lib, self.ctx
        d_in, d_out = C.c_void_p(), C.c_void_p()
        check(lib.ndt_device_alloc(ctx, max(1, n) * 16, C.byref(d_in)), ctx)
        try:
            check(lib.ndt_device_alloc(ctx, max(1, n) * 16, C.byref(d_out)), ctx)
            a4 = np.ascontiguousarray(a[:, :4])
            check(lib.ndt_memcpy_h2d(ctx, d_in, a4.ctypes.data_as(C.c_void_p), n * 16), ctx)
            nout = C.c_size_t()
            rec = _record()
            check(lib.ndt_filter_ground_scan(ctx, C.byref(self._fprm), C.byref(self._gprm), d_in, n, d_out, C.byref(nout), C.byref(rec)), ctx)
            out = np.empty((max(1, nout.value), 4), np.float32)
            check(lib.ndt_memcpy_d2h(ctx, out.ctypes.data_as(C.c_void_p), d_out, nout.value * 16), ctx)
            return out[: nout.value].copy(), GroundResult(self._reg, rec)
        finally:
            lib.ndt_device_free(ctx, d_in)
            if d_out:
                lib.ndt_device_free(ctx, d_out)

    # ------------------------------------------------------------------ test hooks
    def set_samples(self, triples=None):
        """The next detects take these (K, 3) samples in place of the sampler's; None restores the sampler."""
        t = np.zeros((0, 3), np.int32) if triples is None else np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
        check(self._lib.ndt_ground_set_samples(self.ctx, t.ctypes.data_as(_IP), len(t)), self.ctx)

    def last_normals(self):
        """Per point of the last detect's clipped cloud: (normal4 (n, 4): the oriented normal and |n.z|, keep (n,),
        origin (n,): the index in the input cloud, neighbours (n, normal_k))."""
        n = C.c_size_t()
        check(self._lib.ndt_ground_last_normals(self.ctx, None, None, None, None, 0, C.byref(n)), self.ctx)
        m, k = n.value, int(self._gprm.normal_k)
        nrm = np.zeros((max(1, m), 4), np.float32)
        keep, org, nbr = np.zeros(max(1, m), np.int32), np.zeros(max(1, m), np.int32), np.full((max(1, m), k), -1, np.int32)
        check(self._lib.ndt_ground_last_normals(self.ctx, _fp(nrm), keep.ctypes.data_as(_IP), org.ctypes.data_as(_IP),
                                                nbr.ctypes.data_as(_IP), m, C.byref(n)), self.ctx)
        return nrm[:m], keep[:m], org[:m], nbr[:m]

    def last_hypotheses(self):
        """Every hypothesis the last detect's loop looked at: (triples (h, 3), coeffs (h, 4), counts (h,), status (h,))."""
        n = C.c_size_t()
        check(self._lib.ndt_ground_last_hypotheses(self.ctx, None, None, None, None, 0, C.byref(n)), self.ctx)
        h = n.value
        tri, coef = np.zeros((max(1, h), 3), np.int32), np.zeros((max(1, h), 4), np.float32)
        cnt, stat = np.zeros(max(1, h), np.int32), np.zeros(max(1, h), np.int32)
        check(self._lib.ndt_ground_last_hypotheses(self.ctx, tri.ctypes.data_as(_IP), _fp(coef), cnt.ctypes.data_as(_IP),
                                                   stat.ctypes.data_as(_IP), h, C.byref(n)), self.ctx)
        return tri[:h], coef[:h], cnt[:h], stat[:h]

    @property
    def batch(self) -> int:
        """Hypotheses scored per launch."""
        return int(self._lib.ndt_ground_batch())
