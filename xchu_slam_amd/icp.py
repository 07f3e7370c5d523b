"""Host-side mirror of pcl::IterativeClosestPoint<PointXYZI, PointXYZI> and of pgo_node's loop-closure refinement,
backed by libndt_hip.so (include/ndt_hip.h, ndt_icp_*; kernels in csrc/icp.hip).

pgo_node drives the operator in PGO::ICPRefine (/root/reference/xchu_mapping/src/pgo_node.cpp:404-483):

    icp = IterativeClosestPoint()
    icp.setMaxCorrespondenceDistance(150); icp.setMaximumIterations(100)
    icp.setTransformationEpsilon(1e-6); icp.setEuclideanFitnessEpsilon(1e-6); icp.setRANSACIterations(0)
    icp.setInputSource(cureKeyframeCloud); icp.setInputTarget(targetKeyframeCloud)
    icp.align(); icp.hasConverged(); icp.getFitnessScore(); icp.getFinalTransformation()

`refine_loop` restates the whole step (both submaps built on the device) without ROS or GTSAM.  PCL itself is not
available to compare against: the semantics are the restatement in DESIGN.md (parity unpinned).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._ctxobj import _CtxObject
from ._lib import IcpParams, IcpRecord, IcpResult, check
from .ndt import NormalDistributionsTransform, _fp

__all__ = ["IterativeClosestPoint", "refine_loop", "get_transformation", "ICP_STATES"]

ICP_STATES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")


class IterativeClosestPoint(_CtxObject):
    """pcl::IterativeClosestPoint on MI355X.  The operator runs on a registration context: its own, or the one of an
    existing NormalDistributionsTransform (`registration=`), whose target, source and nearest-neighbour index it then
    shares (the context's resolution is the index cell size)."""

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None):
        super().__init__(device, registration)
        self._params = self._default_params(IcpParams, "ndt_icp_default_params", {})
        self._result = IcpResult()
        self._has_result = False

    # ------------------------------------------------------------------ parameters (pcl::Registration)
    def setMaxCorrespondenceDistance(self, d: float):
        self._params.max_corr_dist = float(d)

    def getMaxCorrespondenceDistance(self) -> float:
        return float(self._params.max_corr_dist)

    def setMaximumIterations(self, n: int):
        self._params.max_iter = int(n)

    def getMaximumIterations(self) -> int:
        return int(self._params.max_iter)

    def setTransformationEpsilon(self, eps: float):
        self._params.trans_eps = float(eps)

    def setEuclideanFitnessEpsilon(self, eps: float):
        self._params.fit_eps = float(eps)

    def setRANSACIterations(self, n: int):
        # PCL 1.7's IterativeClosestPoint installs no correspondence rejector: the value has no effect (pgo_node sets 0)
        self.ransac_iterations = int(n)

    def setResolution(self, resolution: float):
        """Cell size of the nearest-neighbour index (the registration context's resolution); not a PCL setting."""
        self._reg.setResolution(resolution)

    # ------------------------------------------------------------------ inputs
    def setInputSource(self, cloud):
        self._reg.setInputSource(cloud)
        self._has_result = False

    def setInputTarget(self, cloud, is_dense: bool = True):
        self._reg.setInputTarget(cloud, is_dense)
        self._has_result = False

    def setInputSourceDevice(self, d_ptr: int, n: int):
        self._reg.setInputSourceDevice(d_ptr, n)
        self._has_result = False

    def setInputTargetDevice(self, d_ptr: int, n: int, is_dense: bool = True):
        self._reg.setInputTargetDevice(d_ptr, n, is_dense)
        self._has_result = False

    # ------------------------------------------------------------------ alignment
    def align(self, guess=None, want_output: bool = True):
        """pcl::Registration::align(output, guess): returns the source transformed by the final transformation."""
        g = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, dtype=np.float32)
        if g.shape != (4, 4):
            raise ValueError("guess must be 4x4")
        colmajor = np.ascontiguousarray(g.T).reshape(-1)
        check(self._lib.ndt_icp_align(self.ctx, C.byref(self._params), _fp(colmajor), C.byref(self._result)), self.ctx)
        self._has_result = True
        if not want_output:
            return None
        n = self._reg._n_source
        out = np.empty((n, 4), dtype=np.float32)
        check(self._lib.ndt_get_output(self.ctx, _fp(out), 16), self.ctx)
        return out[:, :3].copy()

    def getFinalTransformation(self) -> np.ndarray:
        return np.array(self._result.final_tf, dtype=np.float32).reshape(4, 4).T.copy()

    def hasConverged(self) -> bool:
        return bool(self._result.converged)

    def getConvergenceState(self) -> int:
        return int(self._result.state)

    def getFinalNumIteration(self) -> int:
        return int(self._result.nr_iterations)

    def getFitnessScore(self, max_range: float = float(np.finfo(np.float64).max), T=None, return_distances: bool = False):
        """pcl::Registration::getFitnessScore (pgo_node.cpp:441): T defaults to this align's final transformation."""
        return self._reg.getFitnessScore(max_range, T, return_distances)

    def result(self) -> dict:
        r = self._result
        return {"final_tf": self.getFinalTransformation(), "converged": bool(r.converged), "state": int(r.state),
                "nr_iterations": int(r.nr_iterations), "mse": float(r.mse), "n_pairs": int(r.n_pairs)}

    def history(self) -> list[dict]:
        """One record per iteration: incremental transform T, pair count, mse, convergence state."""
        n = C.c_int()
        check(self._lib.ndt_icp_history(self.ctx, None, 0, C.byref(n)), self.ctx)
        recs = (IcpRecord * max(1, n.value))()
        check(self._lib.ndt_icp_history(self.ctx, recs, n.value, C.byref(n)), self.ctx)
        return [{"T": np.array(recs[i].T, dtype=np.float32).reshape(4, 4).T.copy(), "pairs": int(recs[i].n_pairs),
                 "mse": float(recs[i].mse), "state": int(recs[i].state)} for i in range(n.value)]

    def correspondences(self):
        """Test hook: (matched target index per source point, -1 = rejected; squared nearest distance) of the last
        iteration run."""
        n = self._reg._n_source
        idx = np.full(max(n, 1), -1, np.int32)
        d2 = np.zeros(max(n, 1), np.float32)
        nout = C.c_size_t()
        check(self._lib.ndt_icp_correspondences(self.ctx, idx.ctypes.data_as(C.POINTER(C.c_int)), _fp(d2), n, C.byref(nout)), self.ctx)
        return idx[:n], d2[:n]

    def timings(self) -> dict:
        return self._reg.timings()


def get_transformation(x, y, z, roll, pitch, yaw) -> np.ndarray:
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) as an Eigen::Affine3f (pcl/common/impl/eigen.hpp), f32."""
    f = np.float32
    A, B = np.cos(f(yaw)), np.sin(f(yaw))
    Cc, D = np.cos(f(pitch)), np.sin(f(pitch))
    E, F = np.cos(f(roll)), np.sin(f(roll))
    DE, DF = D * E, D * F
    t = np.eye(4, dtype=np.float32)
    t[0, 0] = A * Cc; t[0, 1] = A * DF - B * E; t[0, 2] = B * F + A * DE; t[0, 3] = f(x)
    t[1, 0] = B * Cc; t[1, 1] = A * E + B * DF; t[1, 2] = B * DE - A * F; t[1, 3] = f(y)
    t[2, 0] = -D; t[2, 1] = Cc * F; t[2, 2] = Cc * E; t[2, 3] = f(z)
    return t


def _submap_device(reg: NormalDistributionsTransform, keyframes, poses, idxs, leaf: float):
    """LoopFindNearKeyframesCloud (pgo_node.cpp:530-554) on the device: every keyframe transformed by its pose
    (TransformCloud2Map :568-588, f32), concatenated in index order, pcl::VoxelGrid(leaf).  Returns (device pointer of
    the float4 submap, its point count, device pointers to free)."""
    lib = reg._lib
    clouds = [np.ascontiguousarray(keyframes[i], dtype=np.float32) for i in idxs]
    for a in clouds:
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("keyframes must be (N, 4) x,y,z,intensity arrays")
    total = int(sum(a.shape[0] for a in clouds))
    if total == 0:
        return 0, 0, []
    d_in, d_out = C.c_void_p(), C.c_void_p()
    check(lib.ndt_device_alloc(reg.ctx, total * 16, C.byref(d_in)), reg.ctx)
    check(lib.ndt_device_alloc(reg.ctx, total * 16, C.byref(d_out)), reg.ctx)
    off = 0
    for i, a in zip(idxs, clouds):
        if a.shape[0] == 0:
            continue
        part = C.c_void_p(d_in.value + off * 16)
        check(lib.ndt_memcpy_h2d(reg.ctx, part, a.ctypes.data_as(C.c_void_p), a.nbytes), reg.ctx)
        T = np.ascontiguousarray(get_transformation(*poses[i]).T).reshape(-1)
        check(lib.ndt_transform_device(reg.ctx, _fp(T), part, a.shape[0], part), reg.ctx)
        off += a.shape[0]
    n_out = C.c_size_t()
    st = lib.ndt_voxel_downsample_device(reg.ctx, d_in, total, float(leaf), d_out, C.byref(n_out))
    if st == _lib.NDT_EOVERFLOW:
        # pcl::VoxelGrid: leaf too small for the index range, output = input
        return d_in.value, total, [d_in.value, d_out.value]
    check(st, reg.ctx)
    return d_out.value, int(n_out.value), [d_in.value, d_out.value]


def _submap_store(store, poses, idxs, leaf: float):
    """_submap_device from a KeyframeMap: the keyframes are resident, so the submap is one ndt_map_build into a buffer of
    this call's own (the two submaps of a loop live side by side).  Same return value."""
    reg = store.registration
    total = store.count(idxs)
    if total == 0:
        return 0, 0, []
    d_out = C.c_void_p()
    check(reg._lib.ndt_device_alloc(reg.ctx, total * 16, C.byref(d_out)), reg.ctx)
    try:
        n = store.build_into(d_out.value, total, [poses[i] for i in idxs], idxs, leaf)
    except Exception:
        reg._lib.ndt_device_free(reg.ctx, d_out)
        raise
    return d_out.value, n, [d_out.value]


def refine_loop(keyframes, poses, loop_idx: int, curr_idx: int, search_num: int = 25, leaf: float = 0.5,
                score_threshold: float = 0.3, device: int = 0, resolution: float = 1.0, literal_root: bool = False,
                return_clouds: bool = False, store=None, method: str = "icp", gicp_args: dict | None = None) -> dict:
    """PGO::ICPRefine (pgo_node.cpp:404-483) for one loop candidate, without ROS or GTSAM.

    keyframes: list of (N, 4) x,y,z,intensity clouds in their sensor frames; poses: per keyframe (x, y, z, roll, pitch,
    yaw).  The target submap is the keyframes loop_idx - search_num .. loop_idx + search_num (clipped to the range), the
    source the single keyframe curr_idx, each transformed to the map by its pose and voxel-filtered at `leaf`; ICP runs
    with pgo_node's settings (150 m, 100 iterations, both epsilons 1e-6), then getFitnessScore.  The loop is accepted when
    ICP converged and the score is at most score_threshold (a float in the reference: compared as its f32 value).

    literal_root: the reference's LoopFindNearKeyframesCloud never reads its `key` argument (it stacks root_idx + i, and
    :425 passes the loop keyframe as root), so its source cloud is the loop keyframe itself; True reproduces that.

    store: a KeyframeMap that holds the keyframes on the device.  Both submaps are then built from it (one launch each
    plus the VoxelGrid, no upload per loop) and ICP runs on the store's context, whose resolution, target and source it
    sets; `keyframes` may be None and `device` is the store's.  The result is the same, bit for bit.

    method: "icp" (the reference's refinement, the default) or "gicp": GeneralizedIterativeClosestPoint in ICP's place with
    its own defaults (5 m, 200 iterations, epsilons 5e-4 / 2e-3, k 20), overridden by gicp_args (ndt_gicp_params' field
    names: max_corr_dist, max_iter, trans_eps, rot_eps, k_correspondences, gicp_epsilon, max_inner_iter); the same
    acceptance rule.
    """
    if method not in ("icp", "gicp"):
        raise ValueError("method must be 'icp' or 'gicp'")
    if gicp_args and method != "gicp":
        raise ValueError("gicp_args needs method='gicp'")
    n_kf = len(keyframes) if store is None else len(store)
    if not (0 <= loop_idx < n_kf and 0 <= curr_idx < n_kf) or len(poses) != n_kf:
        raise ValueError("loop_idx / curr_idx out of range, or poses do not match keyframes")
    src_key = loop_idx if literal_root else curr_idx
    tgt_idx = [i for i in range(loop_idx - search_num, loop_idx + search_num + 1) if 0 <= i < n_kf]
    if method == "gicp":
        from .gicp import GeneralizedIterativeClosestPoint
        icp = GeneralizedIterativeClosestPoint(device, None if store is None else store.registration)
        icp._with_overrides(icp._params, gicp_args or {})
    else:
        icp = IterativeClosestPoint(device, None if store is None else store.registration)
    reg = icp.registration
    to_free = []
    try:
        reg.setResolution(resolution)
        if store is None:
            d_src, n_src, f1 = _submap_device(reg, keyframes, poses, [src_key], leaf)
            to_free += f1
            d_tgt, n_tgt, f2 = _submap_device(reg, keyframes, poses, tgt_idx, leaf)
            to_free += f2
        else:
            d_src, n_src, f1 = _submap_store(store, poses, [src_key], leaf)
            to_free += f1
            d_tgt, n_tgt, f2 = _submap_store(store, poses, tgt_idx, leaf)
            to_free += f2
        out = {"n_source": n_src, "n_target": n_tgt}
        if return_clouds:
            for name, d, n in (("source_cloud", d_src, n_src), ("target_cloud", d_tgt, n_tgt)):
                a = np.empty((n, 4), np.float32)
                if n:
                    check(reg._lib.ndt_memcpy_d2h(reg.ctx, a.ctypes.data_as(C.c_void_p), C.c_void_p(d), a.nbytes), reg.ctx)
                out[name] = a
        if n_src == 0 or n_tgt == 0:
            # pcl::Registration::initCompute fails on an empty cloud: align is a no-op and the loop is rejected
            out.update(transform=np.eye(4, dtype=np.float32), score=float(np.finfo(np.float64).max), converged=False,
                       accepted=False, iterations=0, state=_lib.ICP_NOT_CONVERGED)
            return out
        if method == "icp":
            icp.setMaxCorrespondenceDistance(150)
            icp.setMaximumIterations(100)
            icp.setTransformationEpsilon(1e-6)
            icp.setEuclideanFitnessEpsilon(1e-6)
            icp.setRANSACIterations(0)
        icp.setInputSourceDevice(d_src, n_src)
        icp.setInputTargetDevice(d_tgt, n_tgt)
        icp.align(want_output=False)
        score = icp.getFitnessScore()
        converged = icp.hasConverged()
        out.update(transform=icp.getFinalTransformation(), score=score, converged=converged,
                   accepted=bool(converged and not score > float(np.float32(score_threshold))), iterations=icp.getFinalNumIteration(),
                   state=icp.getConvergenceState(), history=icp.history())
        return out
    finally:
        check(reg._lib.ndt_synchronize(reg.ctx), reg.ctx)
        for p in to_free:
            reg._lib.ndt_device_free(reg.ctx, C.c_void_p(p))
        icp.close()
