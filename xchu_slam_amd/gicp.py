"""Host-side mirror of pclomp::GeneralizedIterativeClosestPoint<PointXYZI, PointXYZI> (the reference's
include/pclomp/gicp_omp.h), backed by libndt_hip.so (include/ndt_hip.h, ndt_gicp_*; kernels in csrc/gicp.hip).

Plane-to-plane GICP is the usual upgrade over point-to-point ICP for loop-closure refinement on voxel-filtered LiDAR
submaps: `refine_loop(..., method="gicp")` runs it in ICP's place.  The semantics are the restatement in DESIGN.md (GICP
section; parity unpinned): PCL's bfgs.h is not part of the reference tree, so the minimiser is the project's own.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import GicpParams, GicpRecord, GicpResult, check
from .icp import IterativeClosestPoint
from .ndt import NormalDistributionsTransform, _fp

__all__ = ["GeneralizedIterativeClosestPoint", "GICP_STATES", "GICP_MIN_STATUS"]

GICP_STATES = ("NOT_CONVERGED", "ITERATIONS", "DELTA", "NO_CORRESPONDENCES", "SOLVER_FAILED")
GICP_MIN_STATUS = ("RUNNING", "SUCCESS", "NO_PROGRESS", "MAX_INNER", "FAILED")
_DP = C.POINTER(C.c_double)


class GeneralizedIterativeClosestPoint(IterativeClosestPoint):
    """pclomp::GeneralizedIterativeClosestPoint on MI355X: IterativeClosestPoint's inputs, setters and getters with
    GICP's defaults (5 m, 200 iterations, transformation epsilon 5e-4) and its own align.  setEuclideanFitnessEpsilon
    and setRANSACIterations have no effect, as in the reference (its class inherits both from pcl::IterativeClosestPoint
    and GICP's loop reads neither)."""

    _WHAT = "GICP"

    def __init__(self, device: int = 0, registration: NormalDistributionsTransform | None = None):
        super().__init__(device, registration)
        self._params = self._default_params(GicpParams, "ndt_gicp_default_params", {})
        self._result = GicpResult()
        self.euclidean_fitness_epsilon = 0.0

    # ------------------------------------------------------------------ parameters
    def setEuclideanFitnessEpsilon(self, eps: float):
        self.euclidean_fitness_epsilon = float(eps)

    def setRotationEpsilon(self, eps: float):
        self._params.rot_eps = float(eps)

    def getRotationEpsilon(self) -> float:
        return float(self._params.rot_eps)

    def setCorrespondenceRandomness(self, k: int):
        self._params.k_correspondences = int(k)

    def getCorrespondenceRandomness(self) -> int:
        return int(self._params.k_correspondences)

    def setMaximumOptimizerIterations(self, n: int):
        self._params.max_inner_iter = int(n)

    def getMaximumOptimizerIterations(self) -> int:
        return int(self._params.max_inner_iter)

    # ------------------------------------------------------------------ alignment
    def align(self, guess=None, want_output: bool = True):
        """pcl::Registration::align(output, guess): returns the source transformed by the final transformation."""
        g = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, dtype=np.float32)
        if g.shape != (4, 4):
            raise ValueError("guess must be 4x4")
        colmajor = np.ascontiguousarray(g.T).reshape(-1)
        check(self._lib.ndt_gicp_align(self.ctx, C.byref(self._params), _fp(colmajor), C.byref(self._result)), self.ctx)
        self._has_result = True
        if not want_output:
            return None
        n = self._reg._n_source
        out = np.empty((n, 4), dtype=np.float32)
        check(self._lib.ndt_get_output(self.ctx, _fp(out), 16), self.ctx)
        return out[:, :3].copy()

    def result(self) -> dict:
        r = self._result
        return {"final_tf": self.getFinalTransformation(), "converged": bool(r.converged), "state": int(r.state),
                "nr_iterations": int(r.nr_iterations), "f": float(r.f), "n_pairs": int(r.n_pairs), "n_evals": int(r.n_evals)}

    def history(self) -> list[dict]:
        """One record per outer iteration: transformation_ after it, pairs, f, inner iterations, evaluations, the
        minimiser's status, delta and the convergence state."""
        n = C.c_int()
        check(self._lib.ndt_gicp_history(self.ctx, None, 0, C.byref(n)), self.ctx)
        recs = (GicpRecord * max(1, n.value))()
        check(self._lib.ndt_gicp_history(self.ctx, recs, n.value, C.byref(n)), self.ctx)
        return [{"T": np.array(recs[i].T, dtype=np.float32).reshape(4, 4).T.copy(), "pairs": int(recs[i].n_pairs),
                 "f": float(recs[i].f), "inner": int(recs[i].inner_iterations), "evals": int(recs[i].n_evals),
                 "status": int(recs[i].min_status), "delta": float(recs[i].delta), "state": int(recs[i].state)}
                for i in range(n.value)]

    def covariances(self, which: str = "target", raw: bool = False) -> np.ndarray:
        """Test hook: the (n, 3, 3) covariances of the "target" or "source" under the current k and epsilon; raw: before
        the SVD."""
        w = {"target": 0, "source": 1}[which]
        n = C.c_size_t()
        check(self._lib.ndt_gicp_covariances(self.ctx, C.byref(self._params), w, int(raw), None, 0, C.byref(n)), self.ctx)
        out = np.empty((n.value, 3, 3), np.float64)
        check(self._lib.ndt_gicp_covariances(self.ctx, C.byref(self._params), w, int(raw), out.ctypes.data_as(_DP), n.value,
                                             C.byref(n)), self.ctx)
        return out

    def correspondences(self):
        """Test hook: (matched target index per source point, -1 = rejected; squared nearest distance; M_i (n, 3, 3),
        valid where matched) of the last outer iteration."""
        n = self._reg._n_source
        idx = np.full(max(n, 1), -1, np.int32)
        d2 = np.zeros(max(n, 1), np.float32)
        M = np.zeros((max(n, 1), 3, 3), np.float64)
        nout = C.c_size_t()
        check(self._lib.ndt_gicp_correspondences(self.ctx, idx.ctypes.data_as(C.POINTER(C.c_int)), _fp(d2), M.ctypes.data_as(_DP), n,
                                                 C.byref(nout)), self.ctx)
        return idx[:n], d2[:n], M[:n]

    def evaluate(self, x):
        """Test hook: (f, g[6]) of the last outer iteration's pairs at x = (x, y, z, roll, pitch, yaw), one launch."""
        xv = np.ascontiguousarray(x, np.float64).reshape(6)
        f = C.c_double()
        g = np.zeros(6, np.float64)
        check(self._lib.ndt_gicp_evaluate(self.ctx, xv.ctypes.data_as(_DP), C.byref(f), g.ctypes.data_as(_DP)), self.ctx)
        return float(f.value), g

    def run_stats(self) -> dict:
        """Profiling hook: kernel launches and host round trips of the last align."""
        a, b = C.c_int(), C.c_int()
        check(self._lib.ndt_gicp_run_stats(self.ctx, C.byref(a), C.byref(b)), self.ctx)
        return {"launches": a.value, "round_trips": b.value}
