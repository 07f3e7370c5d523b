"""The global map of pgo_node on the device, and the files its SaveMap writes, backed by libndt_hip.so
(include/ndt_hip.h, ndt_map_*; kernel in csrc/keyframe_map.hip).

pgo_node builds the same cloud in three places (xchu_mapping/src/pgo_node.cpp): every keyframe moved by
its current pose (TransformCloud2Map :568-588, f32), stacked, pcl::VoxelGrid(0.5):

    SaveMap                      :620-653   every keyframe                 -> finalMap.pcd      KeyframeMap.global_map
    PublishPoseAndFrame          :744-812   every second keyframe          -> /pgo_map          KeyframeMap.preview_map
    LoopFindNearKeyframesCloud   :530-554   root +- 25 keyframes           -> ICP submaps       KeyframeMap.submap

`KeyframeMap` keeps the keyframes on the device once and builds any selection of them in one launch plus the VoxelGrid.
`save_map` writes SaveMap's files with `write_pcd`, `write_tum` and `write_g2o`; the three formats are pinned by the
reference's recorded run (tests/golden/pgo_run_1317618205), pcl::VoxelGrid itself stays the restatement of DESIGN.md.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._ctxobj import _CtxObject
from ._lib import check
from .icp import get_transformation
from .ndt import NormalDistributionsTransform, _fp
from .synth import pose_matrix

__all__ = ["KeyframeMap", "save_map", "write_pcd", "read_pcd", "write_tum", "write_g2o", "read_g2o", "matrix_to_quaternion",
           "VELO2CAMERA"]

_IP = C.POINTER(C.c_int)


def _pose_matrices_f32(poses) -> np.ndarray:
    """Per selected keyframe a Pose6D (x, y, z, roll, pitch, yaw) -> the column-major f32 matrices ndt_map_build takes
    (pcl::getTransformation, as TransformCloud2Map builds them); a 4 x 4 entry is taken as the matrix itself."""
    out = np.empty((len(poses), 16), np.float32)
    for k, p in enumerate(poses):
        p = np.asarray(p)
        T = np.asarray(p, np.float32) if p.shape == (4, 4) else get_transformation(*p)
        out[k] = np.ascontiguousarray(T.T).reshape(-1)
    return out


class KeyframeMap(_CtxObject):
    """The keyframe store of pgo_node (keyframeLaserClouds) on MI355X: (N, 4) x,y,z,intensity clouds in their sensor
    frames, resident in one device arena, and the maps built from them.  It runs on a registration context: its own, or
    the one of an existing NormalDistributionsTransform (`registration=`), whose device and stream it then shares."""

    _DESTROY = "ndt_map_destroy"
    _WHAT = "keyframe map"

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None):
        super().__init__(device, registration)
        m = C.c_void_p()
        check(self._lib.ndt_map_create(self.ctx, C.byref(m)), self.ctx)
        self._handle = m
        self.overflowed = False   # the last build's leaf overflowed pcl::VoxelGrid's index range: result = stacked cloud

    # ------------------------------------------------------------------ the store
    def __len__(self) -> int:
        return int(self._lib.ndt_map_size(self._handle))

    def _ll(self, fn: str) -> int:
        v = C.c_longlong()
        check(getattr(self._lib, fn)(self._handle, C.byref(v)), self.ctx)
        return int(v.value)

    @property
    def num_points(self) -> int:
        return self._ll("ndt_map_points")

    @property
    def capacity(self) -> int:
        """Points the arena has room for before it grows."""
        return self._ll("ndt_map_capacity")

    def reserve(self, points: int):
        check(self._lib.ndt_map_reserve(self._handle, int(points)), self.ctx)

    def add(self, cloud) -> int:
        """A keyframe from an (N, 4) x,y,z,intensity host cloud (N = 0 is legal); returns its index."""
        a = np.ascontiguousarray(cloud, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("a keyframe is an (N, 4) x,y,z,intensity array")
        idx = C.c_int()
        check(self._lib.ndt_map_add(self._handle, _fp(a), a.shape[0], 16, 3, C.byref(idx)), self.ctx)
        return idx.value

    def add_device(self, ptr: int, n: int) -> int:
        """A keyframe from a device-resident float4 cloud (device-to-device copy, no transfer); returns its index."""
        idx = C.c_int()
        check(self._lib.ndt_map_add_device(self._handle, C.c_void_p(ptr), int(n), C.byref(idx)), self.ctx)
        return idx.value

    def keyframe(self, i: int) -> np.ndarray:
        """Keyframe i copied back to the host, (N, 4) f32."""
        n = self.keyframe_device(i)[1]
        out = np.empty((n, 4), np.float32)
        check(self._lib.ndt_map_get_keyframe(self._handle, int(i), _fp(out), n, None), self.ctx)
        return out

    def keyframe_device(self, i: int) -> tuple[int, int]:
        """(device pointer, points) of keyframe i; valid until the next add / reserve."""
        p, n = C.c_void_p(), C.c_size_t()
        check(self._lib.ndt_map_keyframe(self._handle, int(i), C.byref(p), C.byref(n)), self.ctx)
        return int(p.value or 0), int(n.value)

    def count(self, indices=None) -> int:
        """Points of a selection (None: every keyframe): what a caller buffer for build_into must hold."""
        idx, n_sel = self._selection(indices)
        total = C.c_longlong()
        check(self._lib.ndt_map_count(self._handle, idx, n_sel, C.byref(total)), self.ctx)
        return int(total.value)

    def geometry(self) -> dict:
        """The last build's launch: workgroups, threads per workgroup, output points per workgroup, segments."""
        g = (C.c_int * 4)()
        check(self._lib.ndt_map_geometry(self._handle, g), self.ctx)
        return {"workgroups": g[0], "block": g[1], "points_per_workgroup": g[2], "segments": g[3]}

    # ------------------------------------------------------------------ builds
    def _selection(self, indices):
        if indices is None:
            return None, len(self)
        sel = np.ascontiguousarray(indices, np.int32).reshape(-1)
        self._sel = sel   # kept alive for the call
        return sel.ctypes.data_as(_IP), len(sel)

    def _build(self, poses, indices, leaf, d_out, cap) -> int:
        idx, n_sel = self._selection(indices)
        if len(poses) != n_sel:
            raise ValueError("one pose per selected keyframe")
        T = _pose_matrices_f32(poses)
        n_out = C.c_size_t()
        st = self._lib.ndt_map_build(self._handle, idx, _fp(T) if n_sel else None, n_sel, float(leaf), d_out, cap, C.byref(n_out))
        self.overflowed = st == _lib.NDT_EOVERFLOW
        if not self.overflowed:
            check(st, self.ctx)
        return int(n_out.value)

    def build(self, poses, indices=None, leaf: float = 0.5, to_host: bool = True):
        """Keyframes `indices` (None: all, in order; a repeated index is stacked twice), each moved by its entry of
        `poses` (a Pose6D (x, y, z, roll, pitch, yaw) per selected keyframe), stacked in selection order, then
        pcl::VoxelGrid(leaf); leaf 0: the stacked cloud itself.  Returns the (K, 4) f32 map, or with to_host=False
        (device pointer, K) of the map's own result buffer (valid until the next build).  `.overflowed` is set when
        the leaf overflowed pcl::VoxelGrid's index range; the result is then the stacked cloud."""
        n = self._build(poses, indices, leaf, None, 0)
        if not to_host:
            p, k = C.c_void_p(), C.c_size_t()
            check(self._lib.ndt_map_result(self._handle, C.byref(p), C.byref(k)), self.ctx)
            return int(p.value or 0), int(k.value)
        out = np.empty((n, 4), np.float32)
        check(self._lib.ndt_map_get(self._handle, _fp(out), n, None), self.ctx)
        return out

    def build_into(self, d_out: int, cap: int, poses, indices=None, leaf: float = 0.5) -> int:
        """`build` into a caller's device buffer with room for cap >= count(indices) points; returns the points written."""
        return self._build(poses, indices, leaf, C.c_void_p(d_out), int(cap))

    # ------------------------------------------------------------------ the reference's three selections
    def global_map(self, poses, leaf: float = 0.5, to_host: bool = True):
        """SaveMap (:620-653): every keyframe.  poses: the Pose6D of every keyframe."""
        self._need_all(poses)
        return self.build(poses, None, leaf, to_host)

    def preview_indices(self, skip: int = 2) -> list[int]:
        return list(range(0, len(self) - 1, skip))   # the loop stops one short of the last keyframe (:755)

    def preview_map(self, poses, skip: int = 2, leaf: float = 0.5, to_host: bool = True):
        """PublishPoseAndFrame (:744-812): keyframes 0, skip, 2 skip, ... below len - 1.  poses: the Pose6D of every
        keyframe."""
        self._need_all(poses)
        idx = self.preview_indices(skip)
        return self.build([poses[i] for i in idx], idx, leaf, to_host)

    def submap_indices(self, root: int, search_num: int = 25) -> list[int]:
        return [i for i in range(root - search_num, root + search_num + 1) if 0 <= i < len(self)]

    def submap(self, poses, root: int, search_num: int = 25, leaf: float = 0.5, to_host: bool = True):
        """LoopFindNearKeyframesCloud (:530-554): root - search_num .. root + search_num, clipped to the range.  poses: the
        Pose6D of every keyframe."""
        self._need_all(poses)
        idx = self.submap_indices(root, search_num)
        return self.build([poses[i] for i in idx], idx, leaf, to_host)

    def _need_all(self, poses):
        if len(poses) != len(self):
            raise ValueError("poses do not match the stored keyframes")


# ---------------------------------------------------------------------------------------------- SaveMap's files (host)
# pgo_node.cpp:687-691: KITTI's ground truth is the camera pose, so the lidar pose is moved to the camera
VELO2CAMERA = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, -0.08], [0.0, 0.0, 0.0, 1.0]])

_PCD_HEADER = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
               "COUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA ascii\n")


def write_pcd(path, xyzi):
    """pcl::io::savePCDFile of a PointXYZI cloud (PCD v0.7 ASCII): PCL's eleven header lines, then one `x y z intensity`
    line per point, every value the f32 printed as %.8g."""
    a = np.asarray(xyzi, np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("a cloud is an (N, 4) x,y,z,intensity array")
    with open(path, "w") as f:
        f.write(_PCD_HEADER.format(n=len(a)))
        f.write("".join("%.8g %.8g %.8g %.8g\n" % tuple(row) for row in a.astype(np.float64).tolist()))


def read_pcd(path) -> np.ndarray:
    """The (N, 4) f32 cloud of an ASCII PCD file with the fields x y z intensity."""
    with open(path) as f:
        header = {}
        for line in f:
            if line.startswith("#"):
                continue
            key, _, val = line.strip().partition(" ")
            header[key] = val
            if key == "DATA":
                break
        if header.get("FIELDS") != "x y z intensity" or header.get("DATA") != "ascii":
            raise ValueError(f"{path}: not an ASCII PCD file of x y z intensity")
        n = int(header["POINTS"])
        vals = np.array(f.read().split(), dtype=np.float64)
    if vals.size != 4 * n:
        raise ValueError(f"{path}: {vals.size} values for {n} points")
    return vals.reshape(n, 4).astype(np.float32)


def _as_matrices(poses) -> np.ndarray:
    """(n, 4, 4) f64 from Pose6D rows (Pose6D2Matrix, common.h:64-71) or 4 x 4 matrices."""
    p = np.asarray(poses, np.float64)
    if p.size == 0:
        return np.zeros((0, 4, 4))
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        return p
    if p.ndim == 2 and p.shape[1] == 6:
        return np.stack([pose_matrix(*row) for row in p])
    raise ValueError("poses are Pose6D rows (x, y, z, roll, pitch, yaw) or 4 x 4 matrices")


def matrix_to_quaternion(R) -> tuple[float, float, float, float]:
    """Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl): the trace branch when
    the trace is positive, else the branch of the largest diagonal entry; (x, y, z, w) with the sign that yields."""
    m = np.asarray(R, np.float64)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = [0.0, 0.0, 0.0]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return float(q[0]), float(q[1]), float(q[2]), float(w)


def write_tum(path, times, poses):
    """SaveMap's odom_tum.txt / lidar_odom.txt (:693-735): per pose (Pose6D or 4 x 4, lidar frame) the camera pose
    velo2camera * Pose6D2Matrix(pose), its rotation as Eigen's quaternion; one line `time x y z qx qy qz qw`, every
    number as %.12g (std::setprecision(12)).  times are written as given (the reference subtracts its first stamp)."""
    M = _as_matrices(poses)
    if len(times) != len(M):
        raise ValueError("one time per pose")
    with open(path, "w") as f:
        for t, m in zip(times, M):
            cam = VELO2CAMERA @ m
            row = (float(t), cam[0, 3], cam[1, 3], cam[2, 3]) + matrix_to_quaternion(cam[:3, :3])
            f.write(" ".join("%.12g" % v for v in row) + "\n")


def read_g2o(path) -> np.ndarray:
    """The VERTEX_SE3:QUAT lines of a g2o file as (n, 7) f64 rows x y z qx qy qz qw (vertex i in row i)."""
    rows = []
    with open(path) as f:
        for line in f:
            w = line.split()
            if w and w[0] == "VERTEX_SE3:QUAT":
                if int(w[1]) != len(rows):
                    raise ValueError(f"{path}: vertex {w[1]} out of order")
                rows.append([float(v) for v in w[2:9]])
    return np.array(rows, np.float64).reshape(len(rows), 7)


def write_g2o(path, poses):
    """SaveMap's pose_graph.g2o (gtsam::writeG2o, :740): one `VERTEX_SE3:QUAT i x y z qx qy qz qw` line per pose, every
    number as %g.  Vertices only: the reference resets its factor container after every ISAM2 update, so the graph it
    hands to writeG2o holds no edge, and its recorded file has none.  poses: Pose6D rows, 4 x 4 matrices, or (n, 7)
    x y z qx qy qz qw rows (read_g2o), which are written as they are."""
    p = np.asarray(poses, np.float64)
    if p.ndim == 2 and p.shape[1] == 7:
        rows = p
    else:
        M = _as_matrices(poses)
        rows = np.array([tuple(m[:3, 3]) + matrix_to_quaternion(m[:3, :3]) for m in M], np.float64).reshape(len(M), 7)
    with open(path, "w") as f:
        for i, r in enumerate(rows):
            f.write("VERTEX_SE3:QUAT %d " % i + " ".join("%g" % v for v in r) + "\n")


def save_map(directory, store, poses, times, odom=None, leaf: float = 0.5) -> np.ndarray:
    """PGO::SaveMap (:620-741) into `directory` (created when missing): finalMap.pcd (store.global_map(poses, leaf);
    `store` may also be a ready (N, 4) map), trajectory.pcd (x, y, z of the poses as f32, intensity 0), odom_tum.txt
    (write_tum of times and poses), pose_graph.g2o (write_g2o of the poses) and, when odom = (stamps, per-scan poses) is
    given, lidar_odom.txt.  poses: the Pose6D of every keyframe.  Returns the final map."""
    P = np.asarray(poses, np.float64).reshape(-1, 6)
    final = store.global_map(P, leaf) if isinstance(store, KeyframeMap) else np.asarray(store, np.float32)
    os.makedirs(directory, exist_ok=True)
    traj = np.zeros((len(P), 4), np.float32)
    traj[:, :3] = P[:, :3]
    write_pcd(os.path.join(directory, "trajectory.pcd"), traj)
    write_pcd(os.path.join(directory, "finalMap.pcd"), final)
    write_tum(os.path.join(directory, "odom_tum.txt"), times, P)
    if odom is not None:
        write_tum(os.path.join(directory, "lidar_odom.txt"), odom[0], odom[1])
    write_g2o(os.path.join(directory, "pose_graph.g2o"), P)
    return final
