"""The host rules of pgo_node's Run loop (xa.keyframe_gate, xa.detect_loop_radius, xa.ape / xa.rpe) and the ABI of
ndt_pgo_set_estimate; no GPU.

The gate is pinned: on lidar_odom.txt of the reference's recorded run (tests/golden/pgo_run_1317618205/lidar_odom.npz:
the stamps and positions parsed from it) it must select exactly the keyframes that run's odom_tum.txt records."""
import ctypes
import os
import re

import numpy as np
import pytest

import pgo_node_restate as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
RUN = os.path.join(GOLDEN, "pgo_run_1317618205")


# ---------------------------------------------------------------------------------------------- the keyframe gate
def test_gate_selects_the_recorded_keyframes():
    import xchu_slam_amd as xa
    z = np.load(os.path.join(RUN, "lidar_odom.npz"))
    stamps, pos = z["stamps"], z["positions"]
    assert stamps.shape == (4527,) and pos.shape == (4527, 3) and stamps.dtype == pos.dtype == np.float64
    idx = xa.keyframe_gate(pos)
    assert len(idx) == 1543 and idx[:6].tolist() == [0, 3, 6, 9, 12, 15]
    assert idx.tolist() == R.keyframe_gate(pos)
    rec = np.load(os.path.join(RUN, "recorded.npz"))
    recorded = np.array([float(line.split()[0]) for line in bytes(rec["odom_tum_txt"]).decode().splitlines() if line.strip()])
    assert len(recorded) == 1541
    assert np.array_equal(stamps[idx[:1541]], recorded)            # exactly, stamp for stamp
    # the last two are absent from the record (the run ended first)
    assert np.allclose(stamps[idx[1541:]], [468.8195, 469.0267], atol=1e-4)


def test_gate_hand_cases():
    import xchu_slam_amd as xa
    x = lambda *v: np.array([[a, 0.0, 0.0] for a in v])
    # the first pose is always selected, wherever it is (the accumulator starts at 1 000 000)
    assert xa.keyframe_gate(x(0.0)).tolist() == [0] and xa.keyframe_gate(x(-7.5)).tolist() == [0]
    assert xa.keyframe_gate(np.zeros((0, 3))).tolist() == []
    # strict >: a step of exactly the gap is no keyframe, the next ulp is
    assert xa.keyframe_gate(x(0.0, 2.0)).tolist() == [0]
    assert xa.keyframe_gate(x(0.0, np.nextafter(2.0, 3.0))).tolist() == [0, 1]
    # the movement accumulates across non-keyframes (0.9 + 0.9 + 0.9 > 2) and restarts at a keyframe
    assert xa.keyframe_gate(x(0.0, 0.9, 1.8, 2.7, 3.6, 4.5, 5.4)).tolist() == [0, 3, 6]
    # path length, not displacement: out and back still accumulates
    assert xa.keyframe_gate(x(0.0, 1.5, 0.0)).tolist() == [0, 2]
    # the step is taken from the previous pose received, not from the last keyframe; all three coordinates count
    p = np.array([[0.0, 0, 0], [0.0, 1.2, 0], [0.0, 1.2, 1.2], [0, 0, 0]])
    assert xa.keyframe_gate(p).tolist() == [0, 2]
    assert xa.keyframe_gate(p, gap=1.0).tolist() == [0, 1, 2, 3]
    # Pose6D rows and matrices are read for their positions
    p6 = np.concatenate([p, np.full((4, 3), 0.3)], 1)
    M = np.tile(np.eye(4), (4, 1, 1))
    M[:, :3, 3] = p
    assert xa.keyframe_gate(p6).tolist() == xa.keyframe_gate(M).tolist() == [0, 2]
    for case in (x(0.0, 0.9, 1.8, 2.7, 3.6, 4.5, 5.4), p):
        assert xa.keyframe_gate(case).tolist() == R.keyframe_gate(case)


# ---------------------------------------------------------------------------------------------- loop_method 0
@pytest.mark.parametrize("name,poses,times,want", R.hand_cases(), ids=[c[0] for c in R.hand_cases()])
def test_loop_method_0_hand_cases(name, poses, times, want):
    import xchu_slam_amd as xa
    assert R.radius_candidate(poses, times) == want
    assert xa.detect_loop_radius(poses, times) == want


def test_loop_method_0_random_against_the_restatement():
    """A random walk that crosses itself, every prefix from 25 keyframes on."""
    import xchu_slam_amd as xa
    rng = np.random.default_rng(3)
    poses = np.zeros((120, 6))
    poses[:, :2] = np.cumsum(rng.normal(0, 2.5, (120, 2)), 0)
    poses[:, 2] = rng.normal(0, 5, 120)                      # z is not part of the distance
    times = np.cumsum(rng.uniform(0.5, 3.0, 120))
    got = [xa.detect_loop_radius(poses[:n], times[:n]) for n in range(25, 121)]
    assert got == [R.radius_candidate(poses[:n], times[:n]) for n in range(25, 121)]
    assert sum(1 for g in got if g != -1) >= 20 and got[:5] == [-1] * 5


# ---------------------------------------------------------------------------------------------- ape / rpe
def tum(n=50, seed=0):
    """A curved trajectory with turning orientations as TUM rows."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) * 0.1
    pos = np.stack([10 * np.cos(0.3 * t * 10 / n * 6), 8 * np.sin(0.2 * t * 10 / n * 6), 0.3 * t], 1) + rng.normal(0, 0.01, (n, 3))
    q = rng.normal(size=(n, 4)) * 0.05 + [0, 0, 0.3, 1.0]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([t[:, None], pos, q], 1)


def rigid(seed=1):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q, rng.normal(size=3) * 20


def quat_mul(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def test_ape_rpe_identical_and_rigid_motion(tmp_path):
    import xchu_slam_amd as xa
    from xchu_slam_amd.globalmap import matrix_to_quaternion
    ref = tum()
    a, r = xa.ape(ref, ref), xa.rpe(ref, ref)
    assert a["max"] < 1e-12 and a["rmse"] < 1e-12
    assert a["matched"] == 50 and r["matched"] == 49 and r["max"] < 1e-12
    assert xa.ape(ref, ref, align=False)["max"] == 0.0
    # a rigid motion of the whole estimate (world frame): ape with alignment is blind to it, rpe too
    Rm, tv = rigid()
    est = ref.copy()
    est[:, 1:4] = ref[:, 1:4] @ Rm.T + tv
    qR = np.array(matrix_to_quaternion(Rm))
    est[:, 4:8] = quat_mul(np.tile(qR, (50, 1)), ref[:, 4:8])
    noisy = est.copy()
    noisy[:, 1:4] += np.random.default_rng(5).normal(0, 0.2, (50, 3))
    base = ref.copy()
    base[:, 1:4] = (noisy[:, 1:4] - tv) @ Rm                       # the same noise, not moved
    a0, a1 = xa.ape(base, ref), xa.ape(noisy, ref)
    assert a0["rmse"] > 0.1
    for k in ("rmse", "mean", "max"):
        assert abs(a0[k] - a1[k]) < 1e-9, (k, a0[k], a1[k])
    assert xa.ape(est, ref)["max"] < 1e-9 and xa.rpe(est, ref)["max"] < 1e-9
    assert xa.ape(est, ref, align=False)["rmse"] > 1.0
    # paths are read like arrays
    pe, pr = tmp_path / "est.txt", tmp_path / "ref.txt"
    np.savetxt(pe, noisy, fmt="%.17g")
    np.savetxt(pr, ref, fmt="%.17g")
    assert xa.ape(str(pe), pr) == a1 and xa.rpe(str(pe), str(pr)) == xa.rpe(noisy, ref)


def test_ape_constant_offset_without_alignment():
    import xchu_slam_amd as xa
    ref = tum()
    est = ref.copy()
    est[:, 1:4] += [3.0, -4.0, 12.0]
    a = xa.ape(est, ref, align=False)
    assert all(abs(a[k] - 13.0) < 1e-12 for k in ("rmse", "mean", "max")) and a["matched"] == 50
    assert xa.ape(est, ref)["max"] < 1e-9                         # a translation is a rigid motion
    assert xa.rpe(est, ref)["max"] < 1e-9                         # and leaves every relative pose alone
    # a relative error: one step of the estimate 0.5 m longer shifts everything after it
    step = ref.copy()
    step[20:, 1] += 0.5
    r = xa.rpe(step, ref)
    assert r["matched"] == 49 and abs(r["max"] - 0.5) < 1e-9 and abs(r["rmse"] - 0.5 / 7.0) < 1e-9


def test_association_window():
    import xchu_slam_amd as xa
    from xchu_slam_amd.trajectory import associate
    ref = tum()
    est = ref[::2].copy()
    est[:, 0] += 0.009                                            # inside the 0.01 s window
    ie, ir = associate(est, ref)
    assert ie.tolist() == list(range(25)) and ir.tolist() == list(range(0, 50, 2))
    est[3, 0] = ref[6, 0] + 0.011                                 # outside: dropped
    est[4, 0] = ref[8, 0] - 0.0101
    ie, ir = associate(est, ref)
    assert ie.tolist() == [k for k in range(25) if k not in (3, 4)] and 6 not in ir and 8 not in ir
    assert xa.ape(est, ref, align=False)["matched"] == 23 and xa.rpe(est, ref)["matched"] == 22
    assert len(associate(est, ref, max_diff=0.02)[0]) == 25
    far = ref.copy()
    far[:, 0] += 100.0
    a = xa.ape(far, ref)
    assert a["matched"] == 0 and np.isnan(a["rmse"]) and xa.rpe(far, ref)["matched"] == 0


def test_path_length_of_kitti_00():
    import xchu_slam_amd as xa
    gt = np.load(os.path.join(GOLDEN, "kitti00_gt.npz"))["tum"]
    assert gt.shape == (4541, 8)
    assert abs(xa.ape(gt, gt)["path_length"] - 3724.187) < 5e-4


# ---------------------------------------------------------------------------------------------- the ABI
def test_set_estimate_is_declared_exported_and_bound():
    from xchu_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    assert re.search(r"^ndt_status ndt_pgo_set_estimate\(ndt_pgo\* pgo, int node, const double pose\[16\]\);", hdr, re.M)
    assert int(re.search(r"#define NDT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.ABI_VERSION
    lib = _lib.load()
    assert hasattr(lib, "ndt_pgo_set_estimate")
    restype, argtypes = _lib.SIGNATURES["ndt_pgo_set_estimate"]
    assert restype is ctypes.c_int and len(argtypes) == 3 and argtypes[1] is ctypes.c_int
    # Only the NULL-handle rejection can be seen here: an ndt_pgo is created on an ndt_ctx, and ndt_create needs a device.
    # The bad-node and non-rigid-pose rejections are in tests/test_gpu_pgo_node.py::test_set_estimate.
    pose = np.eye(4).reshape(-1)
    assert lib.ndt_pgo_set_estimate(None, 0, pose.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == _lib.NDT_EINVAL
    assert lib.ndt_pgo_set_estimate(None, 0, None) == _lib.NDT_EINVAL
    import xchu_slam_amd as xa
    assert callable(xa.PoseGraph.set_estimate)
