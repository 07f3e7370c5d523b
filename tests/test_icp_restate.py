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


# ---------------------------------------------------------------------------------------------- exact under ties
def test_bruteforce_equals_the_tree_path_without_ties():
    from helpers import small_pair
    tgt, src, _ = sparse_scene()
    idx, d2, ties = R.correspondences(src, R.Target(tgt))
    assert not ties.any()
    bi, bd, bn = R.nearest_bruteforce(src, tgt)
    assert np.array_equal(bi, idx) and np.array_equal(bd.view(np.uint32), d2.view(np.uint32)) and np.all(bn == 1)
    pair = small_pair(seed=3, n_source=500)
    sub = pair.target[:6000]
    X = R.transform_f32(pair.guess.astype(np.float32), pair.source)
    idx, d2, ties = R.correspondences(X, R.Target(sub))
    assert not ties.any()
    bi, bd, bn = R.nearest_bruteforce(X, sub, chunk_pairs=1 << 16)  # several chunks
    assert np.array_equal(bi, idx) and np.array_equal(bd.view(np.uint32), d2.view(np.uint32)) and np.all(bn == 1)
    # the exact path of icp() is the same align
    a, b = R.icp(src, tgt, max_iter=3), R.icp(src, tgt, max_iter=3, exact=True)
    assert np.array_equal(a["final"], b["final"]) and [h["mse"] for h in a["history"]] == [h["mse"] for h in b["history"]]


def test_four_nearest_cannot_referee_ties():
    """Why the exact path exists: on the tie lattice up to 14 target points share the minimal f32 distance, and the
    tree's 4 nearest need not hold the lowest index among them; 16 do."""
    import icp_edge_scenes as S
    tgt, q, _ = S.lattice_scene()
    bi, bd, bn = R.nearest_bruteforce(q, tgt)
    assert (bn > 1).sum() >= 1000 and bn.max() > 4
    tree = R.Target(tgt)
    i4, d4, _ = R.correspondences(q, tree, k=4)
    i16, d16, _ = R.correspondences(q, tree, k=16)
    assert np.array_equal(d4.view(np.uint32), bd.view(np.uint32)) and np.array_equal(d16.view(np.uint32), bd.view(np.uint32))
    share4 = float((i4 == bi).mean())
    print("k = 4 returns the lowest index for", share4, "of", len(q), "queries; tied", int((bn > 1).sum()), "most", int(bn.max()))
    assert share4 < 0.95
    assert np.array_equal(i16, bi)


def test_bruteforce_six_duplicates_lowest_index():
    near = [1.5, -2.0, 0.25]
    tgt = np.array([[9, 9, 9], near, [0, 8, 0], near, near, [-7, 0, 1], near, near, near, [1.5, -2.0, 3.0]], np.float32)
    order = np.array([4, 9, 1, 7, 0, 8, 2, 6, 3, 5])  # shuffled: the duplicates land at 0, 2, 3, 5, 7, 8
    P = tgt[order]
    dup = np.flatnonzero((P == np.float32(near)).all(1))
    assert list(dup) == [0, 2, 3, 5, 7, 8]
    q = np.array([[1.5, -2.0, 0.0], near], np.float32)
    idx, d2, count = R.nearest_bruteforce(q, P[::-1])
    assert list(idx) == [len(P) - 1 - dup.max()] * 2 and list(d2) == [0.0625, 0.0] and list(count) == [6, 6]
    idx, d2, ties = R.correspondences(q, R.Target(P), exact=True)
    assert list(idx) == [0, 0] and list(d2) == [0.0625, 0.0] and ties.all()
    r = R.icp(np.repeat(q, 2, 0), P, max_iter=1, exact=True)
    assert list(r["history"][0]["index"]) == [0, 0, 0, 0]


def test_umeyama_reflection_and_ranks():
    """det(sigma) < 0 takes the s = -1 branch and still yields a rotation; rank 2, 1 and 0 cross-covariances yield
    rotations that fit the pairs."""
    import icp_edge_scenes as S
    tgt, src, _ = S.reflection_scene()
    assert np.linalg.det(S.sigma_of(src, tgt)) < 0
    U, _, Vt = np.linalg.svd(S.sigma_of(src, tgt))
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0
    T = R.umeyama(src, tgt).astype(np.float64)
    assert np.linalg.det(T[:3, :3]) > 0 and np.max(np.abs(T - np.asarray(S.rigid(0.2, -0.2, 0.0, 2.0)))) < 1e-3
    for tgt, src, rank in [(*S.planar_partner_scene(5, 0.0), 2), (*S.collinear_scene(), 1), (*S.one_target_scene(), 0)]:
        Q = np.repeat(tgt, len(src), 0) if len(tgt) == 1 else tgt
        assert np.linalg.matrix_rank(S.sigma_of(src, Q), tol=1e-9) == rank
        T = R.umeyama(src, Q).astype(np.float64)
        assert np.max(np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3))) < 1e-6 and np.linalg.det(T[:3, :3]) > 0
        if rank:
            assert S.residual_rms(T, src, Q) < 1e-5  # the partners are a rigid motion apart
        if rank == 2:  # R is unique: extended precision moves no f32 entry by more than one spacing
            Tl = R.umeyama(src, Q, np.longdouble)
            assert np.all(np.abs(Tl.astype(np.float64) - T) <= np.spacing(np.abs(Tl)) + 1e-12)


def test_edge_scene_input_conditions():
    """The reference-side conditions the device tests of tests/test_gpu_icp_edges.py rest on."""
    import icp_edge_scenes as S
    for spacing in (1, 2):
        tgt, q, kinds = S.lattice_scene(spacing=spacing)
        census = S.tie_census(q, tgt, 1.0)
        assert census["tied"].sum() >= 1000 and census["not_first"].sum() >= 100
        if spacing == 2:
            # centre queries whose winner shares a lane with an earlier-scanned candidate in the radius-1 cube: cells
            # 18 and 24 of the 27 follow cells 2 and 8 in lanes 2 and 8
            ct, _ = S.cells_of(tgt, census["geo"])
            cq, _ = S.cells_of(q, census["geo"])
            o = ct[census["winner"]] - cq + 1
            k = o[:, 0] + 3 * o[:, 1] + 9 * o[:, 2]
            assert ((kinds == 0) & np.isin(k, (18, 24))).sum() >= 100
    tgt, src = S.doubled_cell_scene()
    geo = S.index_geometry(tgt, 0.1)
    assert geo["doublings"] == 1 and geo["keys"][0] > 1 << 25 >= geo["keys"][1]
    assert not R.icp(src, tgt, max_iter=1, k=16)["history"][0]["ties"].any()
    for name, tgt in S.shape_targets().items():
        q, c, r0, geo = S.queries_around(tgt, 1.0)
        for axis in range(3):
            for off in (1, 2, 3, 20):
                assert np.any(c[:, axis] == -off) and np.any(c[:, axis] == geo["div_b"][axis] - 1 + off), (name, axis, off)
