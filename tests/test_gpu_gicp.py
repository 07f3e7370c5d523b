"""Generalized-ICP on the device (xa.GeneralizedIterativeClosestPoint, refine_loop(method="gicp")) against
tests/gicp_restate.py.  The scene is tests/test_gpu_icp.py's: helpers.small_pair at index resolution 1.0, the source in
its sensor frame with pair.guess as the guess, or moved to the map frame with an identity guess.

Measured on the MI355X (profiles/gicp.md): whole aligns differ from the restatement by 0 (both forms); the restatement's
own spread under the order of its pair sums is 0 as well, so the bar of test_full_align is TF_TOL.
"""
import numpy as np
import pytest

import gicp_restate as G
import icp_restate as R
from helpers import TF_TOL, X_TOL, small_pair

pytestmark = pytest.mark.gpu

NDT_EINVAL = 1


@pytest.fixture(scope="module")
def scene():
    pair = small_pair(seed=3, n_source=4200)
    tgt = R.Target(pair.target)
    guess = pair.guess.astype(np.float32)
    src_map = R.transform_f32(guess, pair.source)
    nn_t, d2_t, nxt_t = G.knn_order(tgt.pts, 20)
    cov_t, raw_t, s_t = G.covariances(tgt.pts, nn=nn_t)
    return {"pair": pair, "tgt": tgt, "guess": guess, "src_map": src_map, "cov_tgt": cov_t, "raw_tgt": raw_t, "s_tgt": s_t,
            "d2_tgt": d2_t, "nxt_tgt": nxt_t}


def make_gicp(xa, target, source, resolution=1.0, **prm):
    g = xa.GeneralizedIterativeClosestPoint()
    g.setResolution(resolution)
    g.setInputTarget(target)
    g.setInputSource(source)
    configure(g, **prm)
    return g


def configure(g, max_corr_dist=None, max_iter=None, k_correspondences=None):
    if max_corr_dist is not None:
        g.setMaxCorrespondenceDistance(max_corr_dist)
    if max_iter is not None:
        g.setMaximumIterations(max_iter)
    if k_correspondences is not None:
        g.setCorrespondenceRandomness(k_correspondences)


def check_cov(dev_raw, dev_reg, raw, reg, s, max_excluded=0.01):
    """Raw covariances to 1e-12 of their largest entry; regularised ones to 1e-9 where the two smallest singular values
    are apart, and finite, symmetric with eigenvalues (1, 1, 1e-3) everywhere."""
    scale = np.max(np.abs(raw), axis=(1, 2))
    err = np.max(np.abs(dev_raw - raw), axis=(1, 2))
    print("raw worst relative", float(np.max(err / np.maximum(scale, 1e-300))))
    assert np.all(err <= X_TOL * scale)
    apart = (s[:, 1] - s[:, 2]) >= 1e-3 * s[:, 0]
    share = 1.0 - float(np.mean(apart))
    print("excluded share", share)
    assert share <= max_excluded
    e2 = np.max(np.abs(dev_reg - reg), axis=(1, 2))
    print("regularised worst", float(np.max(e2[apart])) if apart.any() else 0.0)
    assert np.all(e2[apart] <= 1e-9)
    assert np.all(np.isfinite(dev_reg))
    assert np.max(np.abs(dev_reg - dev_reg.transpose(0, 2, 1))) <= 1e-9
    ev = np.linalg.eigvalsh(0.5 * (dev_reg + dev_reg.transpose(0, 2, 1)))
    assert np.max(np.abs(ev - np.array([1e-3, 1.0, 1.0]))) <= 1e-9


# ---------------------------------------------------------------------------------------------- 1. covariances
def test_covariances(scene):
    import xchu_slam_amd as xa
    pair = scene["pair"]
    # input conditions: ring 2 and the block shells both run (20th neighbours beyond 2 m and beyond 4 m), no tie at the
    # 20th / 21st neighbour, no point excluded
    nn_s, d2_s, nxt_s = G.knn_order(pair.source, 20)
    reg_s, raw_s, s_s = G.covariances(pair.source, nn=nn_s)
    assert np.sqrt(scene["d2_tgt"][:, -1].max()) > 4.0 and np.sqrt(d2_s[:, -1].max()) > 4.0
    assert not np.any(scene["d2_tgt"][:, -1] == scene["nxt_tgt"]) and not np.any(d2_s[:, -1] == nxt_s)
    with make_gicp(xa, pair.target, pair.source) as g:
        check_cov(g.covariances("target", raw=True), g.covariances("target"), scene["raw_tgt"], scene["cov_tgt"], scene["s_tgt"])
        check_cov(g.covariances("source", raw=True), g.covariances("source"), raw_s, reg_s, s_s)


# ---------------------------------------------------------------------------------------------- 2. ties and duplicates
def lattice():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    dup = g[np.random.default_rng(2).permutation(len(g))[:30]]
    return np.concatenate([g, dup]).astype(np.float32)


def test_ties_and_duplicates():
    import xchu_slam_amd as xa
    pts = lattice()
    nn, d2 = G.knn_bruteforce(pts, 20)
    assert np.any(d2[:, -1] == np.sort(R.l2_simple_f32(pts[None], pts[:, None]), 1)[:, 20])  # ties across the cut
    _, raw, _ = G.covariances(pts, nn=nn)
    with make_gicp(xa, pts, pts) as g:
        for which in ("target", "source"):
            dev = g.covariances(which, raw=True)
            scale = np.max(np.abs(raw), axis=(1, 2))
            assert np.all(np.max(np.abs(dev - raw), axis=(1, 2)) <= X_TOL * scale)
            assert np.all(np.isfinite(g.covariances(which)))


# ---------------------------------------------------------------------------------------------- 3. cloud-size edges
def raw_matches(xa, pts, k=20):
    nn = G.knn_bruteforce(pts, k)[0] if len(pts) <= 3000 else G.knn_order(pts, k)[0]
    _, raw, _ = G.covariances(pts, k, nn=nn)
    with make_gicp(xa, pts, pts, k_correspondences=k) as g:
        dev = g.covariances("source", raw=True)
        reg = g.covariances("source")
    scale = np.maximum(np.max(np.abs(raw), axis=(1, 2)), 1e-300)
    assert dev.shape == raw.shape
    assert np.all(np.max(np.abs(dev - raw), axis=(1, 2)) <= X_TOL * scale)
    assert np.all(np.isfinite(reg))


@pytest.mark.parametrize("n", [20, 21, 31, 32, 33, 4097])
def test_cov_point_counts(scene, n):
    """Exactly k points, one more; one below, at and above two workgroups of 16 teams; and 257 workgroups."""
    import xchu_slam_amd as xa
    raw_matches(xa, scene["src_map"][:n])


@pytest.mark.parametrize("n", [15, 16, 17])
def test_cov_one_workgroup_edge(scene, n):
    """One below, at and above one workgroup's 16 teams (k = 10, so that the cloud may be that small)."""
    import xchu_slam_amd as xa
    raw_matches(xa, scene["src_map"][:n], k=10)


@pytest.mark.parametrize("n", [131071, 131072, 131073])
def test_cov_grid_cap(scene, n):
    """k_gicp_cov's grid is capped at kGicpCovMaxBlocks = 8192 workgroups of 16 teams: one below, at and above the
    131 072 points one trip of its grid-stride loop covers (three copies of the target side by side, 100 m apart)."""
    import xchu_slam_amd as xa
    tgt = scene["pair"].target
    tiled = np.concatenate([tgt + np.array([100.0 * i, 0.0, 0.0], np.float32) for i in range(3)]).astype(np.float32)
    raw_matches(xa, tiled[:n])


@pytest.mark.parametrize("k,n", [(21, 500), (32, 500), (32, 32), (32, 33)])
def test_cov_k_above_20(scene, k, n):
    """k above 20 runs the 32-key instantiation of k_gicp_cov: the first such k, the largest, and the largest on clouds of
    exactly k and k + 1 points."""
    import xchu_slam_amd as xa
    raw_matches(xa, scene["src_map"][:n], k=k)


def test_align_k32(scene):
    """One outer iteration with k = 32 covariances on both clouds against the restatement."""
    import xchu_slam_amd as xa
    check_one_iteration(xa, scene, scene["src_map"][:600], k=32)


def expect_einval(call):
    from xchu_slam_amd._lib import NdtError
    with pytest.raises(NdtError) as e:
        call()
    assert e.value.status == NDT_EINVAL


def test_k_and_cloud_size_limits(scene):
    """k = 33 and a cloud of k - 1 points (source or target) are NDT_EINVAL, from the covariance hook and from align."""
    import xchu_slam_amd as xa
    pts = scene["src_map"]
    with make_gicp(xa, pts[:500], pts[:500], k_correspondences=33) as g:
        expect_einval(lambda: g.covariances("source"))
        expect_einval(lambda: g.covariances("target"))
        expect_einval(g.align)
    with make_gicp(xa, pts[:500], pts[:19]) as g:  # k - 1 source points
        expect_einval(lambda: g.covariances("source"))
        expect_einval(g.align)
        assert g.covariances("target").shape == (500, 3, 3)
    with make_gicp(xa, pts[:19], pts[:500]) as g:  # k - 1 target points
        expect_einval(lambda: g.covariances("target"))
        expect_einval(g.align)
    with make_gicp(xa, pts[:500], pts[:31], k_correspondences=32) as g:
        expect_einval(lambda: g.covariances("source"))
        expect_einval(g.align)


@pytest.mark.parametrize("n_cluster", [20, 19])
def test_cov_far_cluster(scene, n_cluster):
    """A cluster 15 m outside the main cloud's bounding box: with 20 points every neighbour is in the cluster, with 19
    the 20th is in the main cloud."""
    import xchu_slam_amd as xa
    main = scene["src_map"][:1500]
    rng = np.random.default_rng(4)
    cluster = (np.array([main[:, 0].max() + 15.0, 0.0, 2.0]) + rng.uniform(-0.5, 0.5, (n_cluster, 3))).astype(np.float32)
    pts = np.concatenate([main, cluster]).astype(np.float32)
    nn = G.knn_bruteforce(pts, 20)[0]
    inside = (nn[1500:] >= 1500).all(1)
    assert inside.all() if n_cluster == 20 else not inside.any()
    raw_matches(xa, pts)


# ---------------------------------------------------------------------------------------------- 4. pairs
def check_pairs(g, ref):
    h = ref["history"][0]
    assert not h["ties"].any(), "input condition: no query with two candidates at an equal f32 distance"
    idx, d2, M = g.correspondences()
    assert np.array_equal(idx, h["index"])
    assert np.array_equal(d2.view(np.uint32), h["d2"].view(np.uint32))
    pr = h["pair_set"]
    if pr.m:
        scale = np.max(np.abs(pr.M), axis=(1, 2))
        err = np.max(np.abs(M[pr.sel] - pr.M), axis=(1, 2))
        print("M worst relative", float(np.max(err / scale)))
        assert np.all(err <= 1e-9 * scale)
    assert g.history()[0]["pairs"] == pr.m


@pytest.mark.parametrize("max_corr", [5.0, 0.5])
def test_pairs(scene, max_corr):
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["pair"].source[:3000]
    prm = dict(max_iter=1, max_corr_dist=max_corr)
    ref = G.gicp(src, pair.target, scene["guess"], tgt=scene["tgt"], cov_tgt=scene["cov_tgt"], **prm)
    if max_corr == 0.5:
        rejected = 1.0 - ref["history"][0]["pairs"] / len(src)
        assert 0.1 < rejected < 0.9, rejected
    with make_gicp(xa, pair.target, src, **prm) as g:
        g.align(scene["guess"], want_output=False)
        check_pairs(g, ref)
        assert g.getFinalNumIteration() == 1 and g.getConvergenceState() == G.ITERATIONS and g.hasConverged()


def edge_clouds(n_near):
    """A 40-point target blob and a 40-point source blob 100 m apart, plus n_near source points each 0.25 from a target
    point of its own; source point 0 is exactly 0.5 from its only near target point."""
    rng = np.random.default_rng(6)
    tgt = rng.uniform(-1.0, 1.0, (40, 3)).astype(np.float32)
    src = (rng.uniform(-1.0, 1.0, (40, 3)) + np.array([100.0, 0.0, 0.0])).astype(np.float32)
    t_extra = np.array([[20.0 + 4.0 * i, 30.0, 0.0] for i in range(n_near + 1)], np.float32)
    s_extra = t_extra.copy()
    s_extra[0, 0] += np.float32(0.5)
    s_extra[1:, 1] += np.float32(0.25)
    return np.concatenate([t_extra, tgt]), np.concatenate([s_extra, src])


def test_threshold_is_strict():
    import xchu_slam_amd as xa
    tgt, src = edge_clouds(5)
    assert R.l2_simple_f32(tgt[0], src[0]) == np.float32(0.25)
    with make_gicp(xa, tgt, src, max_iter=1, max_corr_dist=0.5) as g:
        g.align(want_output=False)
        idx, d2, _ = g.correspondences()
        assert d2[0] == np.float32(0.25) and idx[0] == -1           # d2 < 0.25 is false: rejected
        assert list(idx[1:6]) == [1, 2, 3, 4, 5] and np.all(idx[6:] == -1)
    with xa.IterativeClosestPoint() as icp:
        icp.setResolution(1.0)
        icp.setInputTarget(tgt)
        icp.setInputSource(src)
        icp.setMaxCorrespondenceDistance(0.5)
        icp.setMaximumIterations(1)
        icp.align(want_output=False)
        idx, d2 = icp.correspondences()
        assert d2[0] == np.float32(0.25) and idx[0] == 0            # ICP's <= keeps it


def test_three_pairs_is_no_correspondences_four_run():
    import xchu_slam_amd as xa
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = [0.01, -0.02, 0.005]
    for n_near, want in ((3, G.NO_CORRESPONDENCES), (4, None)):
        tgt, src = edge_clouds(n_near)
        src = src[1:]  # without the threshold point
        ref = G.gicp(src, tgt, guess, max_iter=1, max_corr_dist=0.5)
        assert ref["history"][0]["pairs"] == n_near
        with make_gicp(xa, tgt, src, max_iter=1, max_corr_dist=0.5) as g:
            g.align(guess, want_output=False)
            r = g.result()
            assert r["n_pairs"] == n_near
            if want is not None:
                assert (r["state"], r["converged"], r["nr_iterations"]) == (want, False, 0)
                assert np.array_equal(r["final_tf"], guess)
            else:
                assert r["nr_iterations"] == 1 and r["state"] == ref["state"] == G.ITERATIONS
                assert g.history()[0]["evals"] == ref["history"][0]["evals"]


# ---------------------------------------------------------------------------------------------- 5. objective
def test_objective(scene):
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["pair"].source[:3000]
    ref = G.gicp(src, pair.target, scene["guess"], tgt=scene["tgt"], cov_tgt=scene["cov_tgt"], max_iter=1)
    h = ref["history"][0]
    with make_gicp(xa, pair.target, src, max_iter=1) as g:
        g.align(scene["guess"], want_output=False)
        for x in [np.zeros(6)] + h["trials"][:3]:
            f, grad = g.evaluate(x)
            rf, rg = G.objective(h["pair_set"], x)
            scale = max(abs(rf), float(np.max(np.abs(rg))))
            err = max(abs(f - rf), float(np.max(np.abs(grad - rg))))
            print("x", x, "f", f, "relative error", err / scale)
            assert err <= X_TOL * scale


def test_hooks_refuse_a_replaced_source(scene):
    """After setInputSource with another cloud of the same size the last align's pairs are stale: both hooks say so."""
    import xchu_slam_amd as xa
    from xchu_slam_amd._lib import NdtError
    pair = scene["pair"]
    with make_gicp(xa, pair.target, scene["src_map"][:500], max_iter=1) as g:
        g.align(want_output=False)
        g.evaluate(np.zeros(6))
        g.setInputSource(scene["src_map"][500:1000])
        for call in (lambda: g.evaluate(np.zeros(6)), g.correspondences):
            with pytest.raises(NdtError) as e:
                call()
            assert e.value.status == NDT_EINVAL
        g.align(want_output=False)
        g.evaluate(np.zeros(6))


# ---------------------------------------------------------------------------------------------- 6. whole aligns
def restated(scene, src, guess, **prm):
    cov_src = G.covariances(src)[0]
    runs = [G.gicp(src, scene["pair"].target, guess, tgt=scene["tgt"], cov_tgt=scene["cov_tgt"], cov_src=cov_src, pair_order=o,
                   **prm) for o in (None, "reversed", 23)]
    seq = [[(h["pairs"], h["evals"], h["status"]) for h in r["history"]] for r in runs]
    assert seq[0] == seq[1] == seq[2], "input condition: the restatement takes one evaluation sequence under any pair order"
    spread = max(float(np.max(np.abs(r["final"] - runs[0]["final"]))) for r in runs[1:])
    return runs[0], spread


@pytest.mark.parametrize("form", ["sensor_frame_guess", "map_frame_identity"])
def test_full_align(scene, form):
    import xchu_slam_amd as xa
    pair = scene["pair"]
    if form == "sensor_frame_guess":
        src, guess = pair.source[:3000], scene["guess"]
    else:
        src, guess = scene["src_map"][:3000], None
    ref, spread = restated(scene, src, guess)
    with make_gicp(xa, pair.target, src) as g:
        out = g.align(guess)
        r, dev = g.result(), g.history()
        print("iterations", r["nr_iterations"], G.STATE_NAMES[r["state"]], "restatement", ref["iterations"],
              G.STATE_NAMES[ref["state"]], "evals", r["n_evals"], ref["evals"], g.run_stats())
        assert (r["nr_iterations"], r["state"], r["converged"]) == (ref["iterations"], ref["state"], ref["converged"])
        assert [h["pairs"] for h in dev] == [h["pairs"] for h in ref["history"]]
        assert [(h["evals"], h["inner"], h["status"]) for h in dev] == [(h["evals"], h["inner"], h["status"]) for h in ref["history"]]
        assert [h["state"] for h in dev] == [h["state"] for h in ref["history"]]
        assert r["n_evals"] == ref["evals"]
        diff = float(np.max(np.abs(r["final_tf"] - ref["final"])))
        print("restatement spread", spread, "device difference", diff)
        assert diff <= max(TF_TOL, 10.0 * spread)
        assert abs(r["f"] - ref["f"]) <= 1e-6 * abs(ref["f"])
        # getFitnessScore and align's output refer to this align
        T = g.getFinalTransformation()
        assert np.array_equal(out, R.transform_f32(T, src))
        score = R.fitness_score(src, pair.target, T, tgt=scene["tgt"])
        assert abs(g.getFitnessScore() - score) <= 1e-12 * score


def rec_bytes(h):
    return [(x["T"].tobytes(), x["pairs"], x["f"], x["inner"], x["evals"], x["status"], x["delta"], x["state"]) for x in h]


def test_deterministic_and_iteration_cap(scene):
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["src_map"][:3000]
    runs = []
    with make_gicp(xa, pair.target, src) as g:
        for _ in range(2):
            g.align(want_output=False)
            runs.append((rec_bytes(g.history()), g.getFinalTransformation().tobytes()))
        assert len(runs[0][0]) > 2
        assert runs[0] == runs[1]
        g.setMaximumIterations(3)
        g.align(want_output=False)
        assert (g.getFinalNumIteration(), g.getConvergenceState(), g.hasConverged()) == (3, G.ITERATIONS, True)
        assert rec_bytes(g.history())[:2] == runs[0][0][:2]
        g.setMaximumIterations(2)  # the cap cuts the run short
        g.align(want_output=False)
        assert (g.getFinalNumIteration(), g.getConvergenceState(), g.hasConverged()) == (2, G.ITERATIONS, True)
        assert len(g.history()) == 2 and rec_bytes(g.history())[:1] == runs[0][0][:1]
    with make_gicp(xa, pair.target, src) as g:
        g.align(want_output=False)
        assert (rec_bytes(g.history()), g.getFinalTransformation().tobytes()) == runs[0]


def check_one_iteration(xa, scene, src, k=20):
    pair = scene["pair"]
    prm = dict(max_iter=1, k_correspondences=k)
    ref = G.gicp(src, pair.target, tgt=scene["tgt"], cov_tgt=scene["cov_tgt"] if k == 20 else None, **prm)
    with make_gicp(xa, pair.target, src, **prm) as g:
        g.align(want_output=False)
        check_pairs(g, ref)
        d, h = g.history()[0], ref["history"][0]
        assert d["pairs"] == len(src)
        assert (d["evals"], d["inner"], d["status"]) == (h["evals"], h["inner"], h["status"])
        assert np.max(np.abs(g.getFinalTransformation() - ref["final"])) <= TF_TOL


@pytest.mark.parametrize("n_source", [20, 31, 32, 33, 255, 256, 257, 4097])
def test_source_sizes(scene, n_source):
    """Exactly k source points; one below, at and above two workgroups of k_gicp_pairs (16 teams each) and one workgroup
    of k_gicp_eval (256 threads); and 4097 points (17 evaluation workgroups, 257 of the pairs kernel)."""
    import xchu_slam_amd as xa
    check_one_iteration(xa, scene, scene["src_map"][:n_source])


@pytest.mark.parametrize("n_source", [15, 16, 17])
def test_source_one_workgroup_edge(scene, n_source):
    """One below, at and above one workgroup of k_gicp_pairs (k = 10, so that the source may be that small)."""
    import xchu_slam_amd as xa
    check_one_iteration(xa, scene, scene["src_map"][:n_source], k=10)


@pytest.fixture(scope="module")
def big_source(scene):
    """66 000 points of the same sensor pose moved to the map frame, without the few queries that have two candidates
    at an equal f32 distance (check_pairs' input condition)."""
    big = small_pair(seed=3, n_source=66000)
    assert np.array_equal(big.target, scene["pair"].target)
    src = R.transform_f32(scene["guess"], big.source)
    ties = R.correspondences(src, scene["tgt"])[2]
    assert ties.sum() < 100
    return src[~ties]


@pytest.mark.parametrize("n_source", [16383, 16384, 16385, 65536, 65537])
def test_source_grid_caps(scene, big_source, n_source):
    """k_gicp_pairs' grid is capped at kGicpMaxBlocks = 1024 workgroups (16 384 points per trip of its grid-stride
    loop), k_gicp_eval's at kGicpEvalBlocks = 256 (65 536 points): one below, at and above the first, at and above the
    second."""
    import xchu_slam_amd as xa
    check_one_iteration(xa, scene, big_source[:n_source])


# ---------------------------------------------------------------------------------------------- 7. refine_loop
def test_refine_loop_gicp():
    import xchu_slam_amd as xa
    from test_gpu_icp import host_submap, loop_keyframes
    keyframes, poses, true11 = loop_keyframes()
    out = xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, method="gicp")
    src = host_submap(xa, keyframes, poses, [11], 0.5)
    tgt = host_submap(xa, keyframes, poses, [0, 1, 2], 0.5)
    ref = G.gicp(src, tgt)
    print("iterations", out["iterations"], "restatement", ref["iterations"], "score", out["score"])
    assert (out["iterations"], out["state"], out["converged"]) == (ref["iterations"], ref["state"], ref["converged"])
    assert [h["pairs"] for h in out["history"]] == [h["pairs"] for h in ref["history"]]
    assert np.max(np.abs(out["transform"] - ref["final"])) <= TF_TOL
    score = R.fitness_score(src, tgt, out["transform"])
    assert abs(out["score"] - score) <= 1e-12 * score
    assert out["accepted"] == (bool(ref["converged"]) and score <= float(np.float32(0.3)))
    corrected = out["transform"].astype(np.float64) @ R.get_transformation(*poses[11]).astype(np.float64)
    assert np.linalg.norm(corrected[:3, 3] - true11) < 0.15
    # from a KeyframeMap store: identical
    with xa.KeyframeMap() as store:
        for k in keyframes:
            store.add(k)
        out2 = xa.refine_loop(None, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, store=store, method="gicp")
    assert out2["transform"].tobytes() == out["transform"].tobytes() and out2["score"] == out["score"]
    assert rec_bytes(out2["history"]) == rec_bytes(out["history"])
    # gicp_args reach the operator
    out3 = xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, method="gicp",
                          gicp_args=dict(max_iter=1))
    assert out3["iterations"] == 1 and out3["state"] == G.ITERATIONS


def test_refine_loop_icp_unchanged():
    """method="icp" and no method argument: the direct ICP path, bit for bit."""
    import xchu_slam_amd as xa
    from test_gpu_icp import PGO, host_submap, loop_keyframes
    keyframes, poses, _ = loop_keyframes()
    a = xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5)
    b = xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, method="icp")
    src = host_submap(xa, keyframes, poses, [11], 0.5)
    tgt = host_submap(xa, keyframes, poses, [0, 1, 2], 0.5)
    with xa.IterativeClosestPoint() as icp:
        icp.setResolution(1.0)
        icp.setInputTarget(tgt)
        icp.setInputSource(src)
        icp.setMaxCorrespondenceDistance(PGO["max_corr_dist"])
        icp.setMaximumIterations(PGO["max_iter"])
        icp.setTransformationEpsilon(PGO["trans_eps"])
        icp.setEuclideanFitnessEpsilon(PGO["fit_eps"])
        icp.align(want_output=False)
        T, score, it = icp.getFinalTransformation(), icp.getFitnessScore(), icp.getFinalNumIteration()
    for out in (a, b):
        assert out["transform"].tobytes() == T.tobytes() and out["score"] == score and out["iterations"] == it
    with pytest.raises(ValueError):
        xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, method="ndt")
