"""Known answers that pin tests/icp_restate.py (the executable form of the ICP semantics the device is compared with),
and the C layouts of the ICP structs.  No GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np

import icp_restate as R
from conftest import ROOT


def rigid(tx, ty, tz, deg, axis=(0.0, 0.0, 1.0)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T[:3, 3] = [tx, ty, tz]
    return T


def sparse_scene(seed=0, n_target=300, n_source=200, side=40.0):
    """Random points in a cube, mean spacing ~6 m: a 0.3 m / 2 deg displacement leaves every nearest neighbour the
    true partner.  The target is a superset of the source's points."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-side / 2, side / 2, (n_target, 3)).astype(np.float32)
    T = rigid(0.2, -0.2, 0.1, 2.0, (0.2, -0.1, 1.0))  # |t| = 0.3
    inv = np.linalg.inv(T)
    src = (tgt[:n_source].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return tgt, src, T


def test_recovers_a_known_rigid_transform():
    tgt, src, T = sparse_scene()
    r = R.icp(src, tgt, max_iter=10)
    assert r["converged"]
    assert r["history"][0]["pairs"] == len(src)
    assert np.array_equal(r["history"][0]["index"], np.arange(len(src)))  # the first match is already the true partner
    # f32 coordinates of magnitude 10: the source carries 1e-6 of rounding, the estimate averages it down
    assert np.max(np.abs(r["final"].astype(np.float64) - T)) < 5e-6
    assert r["mse"] < 1e-11


def test_state_iterations():
    tgt, src, _ = sparse_scene()
    r = R.icp(src, tgt, max_iter=1, trans_eps=1e-6, fit_eps=1e-6)
    assert (r["state"], r["converged"], r["iterations"]) == (R.ITERATIONS, True, 1)
    assert len(r["history"]) == 1 and r["history"][0]["state"] == R.ITERATIONS


def test_state_transform():
    # the second estimate is the identity up to rounding: cos >= 1 - eps and |t|^2 <= eps
    tgt, src, _ = sparse_scene()
    r = R.icp(src, tgt, max_iter=50, trans_eps=1e-6)
    assert (r["state"], r["converged"], r["iterations"]) == (R.TRANSFORM, True, 2)
    assert [h["state"] for h in r["history"]] == [R.NOT_CONVERGED, R.TRANSFORM]


def test_state_abs_mse():
    # both epsilons off: the mse settles at the f32 rounding floor (~1e-13) and stops changing
    tgt, src, _ = sparse_scene()
    r = R.icp(src, tgt, max_iter=50)
    assert (r["state"], r["converged"]) == (R.ABS_MSE, True)
    assert 2 <= r["iterations"] <= 4


def test_state_rel_mse():
    # a noisy target keeps the mse at the noise floor (3 * 0.05^2 = 0.0075): the first estimate removes the 0.3 m
    # displacement (the mse falls by more than half), the second changes it little, but far more than 1e-12
    tgt, src, _ = sparse_scene(seed=1)
    rng = np.random.default_rng(5)
    noisy = (tgt + rng.normal(0, 0.05, tgt.shape)).astype(np.float32)
    r = R.icp(src, noisy, max_iter=50, fit_eps=0.5)
    assert (r["state"], r["converged"], r["iterations"]) == (R.REL_MSE, True, 3)
    h = r["history"]
    assert [x["state"] for x in h] == [R.NOT_CONVERGED, R.NOT_CONVERGED, R.REL_MSE]
    assert abs(h[1]["mse"] - h[0]["mse"]) / h[0]["mse"] >= 0.5
    assert abs(h[2]["mse"] - h[1]["mse"]) > 1e-12 and abs(h[2]["mse"] - h[1]["mse"]) / h[1]["mse"] < 0.5


def test_two_pairs_is_no_correspondences():
    tgt, src, _ = sparse_scene()
    guess = rigid(0.05, 0.0, 0.0, 0.5).astype(np.float32)
    r = R.icp(src[:2], tgt, guess=guess)
    assert (r["state"], r["converged"], r["iterations"], r["pairs"]) == (R.NO_CORRESPONDENCES, False, 0, 2)
    assert np.array_equal(r["final"], guess)
    # many points, two within the correspondence distance
    far = src.copy()
    far[2:] += np.float32(500.0)
    r = R.icp(far, tgt, max_corr_dist=5.0)
    assert (r["state"], r["converged"], r["pairs"]) == (R.NO_CORRESPONDENCES, False, 2)
    assert np.array_equal(r["final"], np.eye(4, dtype=np.float32))


def test_hand_computed_four_points():
    tgt = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]], np.float32)
    src = np.array([[0.5, 0, 0], [10, 0.25, 0], [0, 10, 1.0], [0, 0, 13]], np.float32)
    # squared distances 0.25, 0.0625, 1, 9 (all exact in f32); 9 > 2^2 is rejected
    r = R.icp(src, tgt, max_corr_dist=2.0, max_iter=1)
    h = r["history"][0]
    assert h["pairs"] == 3 and h["mse"] == (0.25 + 0.0625 + 1.0) / 3
    assert list(h["index"]) == [0, 1, 2, -1] and list(h["d2"]) == [0.25, 0.0625, 1.0, 9.0]
    # d2 == max_corr_dist^2 is kept (<=)
    r = R.icp(src, tgt, max_corr_dist=3.0, max_iter=1)
    assert r["history"][0]["pairs"] == 4 and r["history"][0]["mse"] == (0.25 + 0.0625 + 1.0 + 9.0) / 4


def test_equal_distances_go_to_the_lowest_index():
    tgt = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    idx, d2, ties = R.correspondences(np.zeros((1, 3), np.float32), R.Target(tgt[::-1].copy()))
    assert idx[0] == 1 and d2[0] == 1.0 and ties[0]  # reversed order: indices 1, 2, 3 tie; the lowest wins


def test_icp_struct_layouts(tmp_path):
    """The ctypes mirrors of the ICP structs have the C header's sizes and field offsets."""
    from xchu_slam_amd import _lib
    structs = {"ndt_icp_params": _lib.IcpParams, "ndt_icp_result": _lib.IcpResult, "ndt_icp_record": _lib.IcpRecord}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "ndt_hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        src.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            src.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    p = _lib.IcpParams()
    assert _lib.load().ndt_icp_default_params(ctypes.byref(p)) == 0
    assert p.max_corr_dist == math.sqrt(R.DBL_MAX) and p.max_iter == 10 and p.trans_eps == 0.0 and p.fit_eps == 0.0
