"""Property checks of tests/gicp_restate.py, the executable form of the GICP semantics (no GPU)."""
import numpy as np
import pytest

import gicp_restate as G
import icp_restate as R
from helpers import pose_err, small_pair
from xchu_slam_amd import synth


@pytest.fixture(scope="module")
def scene():
    pair = small_pair(seed=3, n_source=4200)
    tgt = R.Target(pair.target)
    guess = pair.guess.astype(np.float32)
    src_map = R.transform_f32(guess, pair.source)
    return {"pair": pair, "tgt": tgt, "guess": guess, "src_map": src_map, "cov_tgt": G.covariances(tgt.pts)[0]}


def test_covariance_structure(scene):
    """Regularised covariances are symmetric with eigenvalues (1, 1, epsilon); the k-NN order is (d2, index)."""
    pts = scene["src_map"]
    nn, d2, nxt = G.knn_order(pts, 20)
    assert np.array_equal(nn[:, 0], np.arange(len(pts))) and np.all(d2[:, 0] == 0)
    assert np.all(np.diff(d2.astype(np.float64), axis=1) >= 0) and np.all(nxt >= d2[:, -1])
    reg, raw, s = G.covariances(pts, nn=nn)
    assert np.max(np.abs(reg - reg.transpose(0, 2, 1))) < 1e-15
    ev = np.linalg.eigvalsh(reg)
    assert np.max(np.abs(ev - np.array([1e-3, 1.0, 1.0]))) < 1e-9
    with pytest.raises(ValueError):
        G.covariances(pts[:19], 20)


def test_knn_order_matches_bruteforce_under_ties():
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = np.concatenate([g, g[:10]])
    nn, d2, _ = G.knn_order(pts, 20, extra=60)
    bn, bd = G.knn_bruteforce(pts, 20)
    assert np.array_equal(nn, bn) and np.array_equal(d2, bd)


def test_gradient_matches_central_differences(scene):
    """The analytic gradient against central differences (h = 1e-5, f64 transforms), 1e-6 relative, on the pairs the
    first outer iteration finds.  The source is in the map frame (identity guess): with a translating guess the
    reference's rotation gradient multiplies by guess * p, translation included, and is not the derivative — a quirk the
    restatement keeps (GICP)."""
    src = scene["src_map"]
    cov_src = G.covariances(src)[0]
    eye = np.eye(4, dtype=np.float32)
    pr = G.Pairs(src, scene["tgt"], eye, eye, cov_src, scene["cov_tgt"], 5.0)
    assert pr.m > 3000
    h = 1e-5
    for x in (np.zeros(6), np.array([0.05, -0.03, 0.01, 0.004, -0.006, 0.01])):
        f, g = G.objective(pr, x, np.float64)
        num = np.zeros(6)
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            num[k] = (G.objective(pr, x + e, np.float64)[0] - G.objective(pr, x - e, np.float64)[0]) / (2 * h)
        rel = float(np.max(np.abs(num - g)) / np.max(np.abs(g)))
        print("x", x, "f", f, "rel", rel)
        assert rel < 1e-6
        # the literal f32 route is the same function up to f32 rounding of the moved points
        f32v, g32 = G.objective(pr, x)
        assert abs(f32v - f) < 1e-4 * abs(f) and np.max(np.abs(g32 - g)) < 1e-3 * np.max(np.abs(g))


def test_apply_state_quaternion_route():
    x = np.array([0.1, -0.2, 0.3, 0.02, -0.015, 0.4])
    T32, T64 = G.apply_state(np.eye(4, dtype=np.float32), x), G.apply_state(np.eye(4), x, np.float64)
    assert T32.dtype == np.float32 and np.max(np.abs(T32 - T64)) < 3e-7
    Rz_Ry_Rx = synth.pose_matrix(0, 0, 0, x[3], x[4], x[5])[:3, :3] if hasattr(synth, "pose_matrix") else None
    if Rz_Ry_Rx is not None:
        assert np.max(np.abs(T64[:3, :3] - Rz_Ry_Rx)) < 1e-12
    assert np.max(np.abs(G.state_of_transform(T32) - x)) < 1e-6


def test_known_answer(scene):
    pair = scene["pair"]
    assert len(pair.target) == 45480
    Tk = synth.pose_matrix(0.2, -0.15, 0.05, 0.01, -0.008, 0.02)
    sel = np.random.default_rng(5).permutation(len(pair.target))[:3000]
    inv = np.linalg.inv(Tk)
    src = (pair.target[sel].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    out = G.gicp(src, pair.target, tgt=scene["tgt"], cov_tgt=scene["cov_tgt"])
    print("iterations", out["iterations"], G.STATE_NAMES[out["state"]], "evals", out["evals"])
    dt = float(np.max(np.abs(out["final"][:3, 3] - Tk[:3, 3])))
    dr = float(np.max(np.abs(out["final"][:3, :3] - Tk[:3, :3])))
    print("translation", dt, "rotation", dr)
    assert out["converged"] and out["state"] == G.DELTA
    assert dt < 5e-4 and dr < 2e-3


def test_small_pair_map_frame(scene):
    pair = scene["pair"]
    out = G.gicp(scene["src_map"], pair.target, tgt=scene["tgt"], cov_tgt=scene["cov_tgt"])
    t0, r0 = pose_err(scene["guess"], pair.true_pose)
    t1, r1 = pose_err(out["final"].astype(np.float64) @ scene["guess"].astype(np.float64), pair.true_pose)
    print("guess", t0, r0, "->", t1, r1, "iterations", out["iterations"], "evals", out["evals"],
          [G.MIN_NAMES[h["status"]] for h in out["history"]])
    assert out["converged"] and out["state"] == G.DELTA
    assert t1 <= 0.1 * t0 and r1 <= 0.1 * r0


def test_pair_order_spread_is_small(scene):
    """The restatement's own spread under the summation order of the pair sums: same evaluation sequence, final
    transforms within 1e-6."""
    pair, src = scene["pair"], scene["src_map"][:3000]
    cov_src = G.covariances(src)[0]
    runs = [G.gicp(src, pair.target, tgt=scene["tgt"], cov_tgt=scene["cov_tgt"], cov_src=cov_src, pair_order=o)
            for o in (None, "reversed", 17)]
    seq = [[(h["pairs"], h["evals"], h["status"]) for h in r["history"]] for r in runs]
    assert seq[0] == seq[1] == seq[2]
    spread = max(float(np.max(np.abs(r["final"] - runs[0]["final"]))) for r in runs[1:])
    print("spread", spread)
    assert spread < 1e-6


def test_too_few_pairs_and_iteration_cap(scene):
    pair = scene["pair"]
    far = (pair.target[:30] + np.float32(500.0)).astype(np.float32)
    out = G.gicp(far, pair.target, tgt=scene["tgt"], cov_tgt=scene["cov_tgt"])
    assert (out["state"], out["converged"], out["iterations"]) == (G.NO_CORRESPONDENCES, False, 0)
    assert np.array_equal(out["final"], np.eye(4, dtype=np.float32))
    out = G.gicp(scene["src_map"][:1000], pair.target, tgt=scene["tgt"], cov_tgt=scene["cov_tgt"], max_iter=1)
    assert (out["state"], out["converged"], out["iterations"]) == (G.ITERATIONS, True, 1)
