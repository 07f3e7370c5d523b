"""Point-to-point ICP on the device (xa.IterativeClosestPoint, xa.refine_loop) against tests/icp_restate.py.

Scenes: helpers.small_pair (a 40 m half-width world, ~40 k target points) at index resolution 1.0.  The source is used
in two forms: in its sensor frame with pair.guess as the align's guess (the guess transform runs on the device), and
moved to the map frame by pair.guess on the host with an identity guess (pgo_node's form: clouds in the map frame, the
estimate a small correction, every transform entry below 2).
"""
import math

import numpy as np
import pytest

import icp_restate as R
from helpers import TF_TOL, pose_err, small_pair

pytestmark = pytest.mark.gpu

PGO = dict(max_corr_dist=150.0, max_iter=100, trans_eps=1e-6, fit_eps=1e-6)


@pytest.fixture(scope="module")
def scene():
    pair = small_pair(seed=3, n_source=4200)
    tgt = R.Target(pair.target)
    guess = pair.guess.astype(np.float32)
    src_map = R.transform_f32(guess, pair.source)  # map frame, off the truth by the pair's perturbation
    return {"pair": pair, "tgt": tgt, "guess": guess, "src_map": src_map}


def make_icp(xa, target, source, resolution=1.0, **prm):
    icp = xa.IterativeClosestPoint()
    icp.setResolution(resolution)
    icp.setInputTarget(target)
    icp.setInputSource(source)
    configure(icp, **prm)
    return icp


def configure(icp, max_corr_dist=None, max_iter=None, trans_eps=None, fit_eps=None):
    if max_corr_dist is not None:
        icp.setMaxCorrespondenceDistance(max_corr_dist)
    if max_iter is not None:
        icp.setMaximumIterations(max_iter)
    if trans_eps is not None:
        icp.setTransformationEpsilon(trans_eps)
    if fit_eps is not None:
        icp.setEuclideanFitnessEpsilon(fit_eps)


def check_first_iteration(icp, ref):
    """The device's last pass against the restatement's first iteration: match, d2, pairs exact; mse to 1e-12."""
    h = ref["history"][0]
    assert not h["ties"].any(), "input condition: no query with two candidates at an equal f32 distance"
    idx, d2 = icp.correspondences()
    assert np.array_equal(idx, h["index"])
    assert np.array_equal(d2.view(np.uint32), h["d2"].view(np.uint32))
    dev = icp.history()
    assert dev[0]["pairs"] == h["pairs"]
    if h["pairs"]:
        assert abs(dev[0]["mse"] - h["mse"]) <= 1e-12 * h["mse"]
    return dev


@pytest.mark.parametrize("max_corr", [None, 0.5])
def test_correspondences_exact(scene, max_corr):
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["pair"].source[:3000]
    prm = dict(max_iter=1) if max_corr is None else dict(max_iter=1, max_corr_dist=max_corr)
    ref = R.icp(src, pair.target, scene["guess"], tgt=scene["tgt"], **prm)
    if max_corr is not None:
        rejected = 1.0 - ref["history"][0]["pairs"] / len(src)
        assert 0.1 < rejected < 0.9, rejected  # a real share of both kinds
    with make_icp(xa, pair.target, src, **prm) as icp:
        icp.align(scene["guess"], want_output=False)
        dev = check_first_iteration(icp, ref)
        assert icp.getFinalNumIteration() == 1 and icp.getConvergenceState() == R.ITERATIONS and icp.hasConverged()
        assert np.max(np.abs(dev[0]["T"] - ref["history"][0]["T"])) < TF_TOL


def test_far_walk(scene):
    """A 300-point cluster 15 m outside the target's bounding box (query cells outside the grid, block-shell phase) and
    5 points beyond 300 m; identity guess."""
    import xchu_slam_amd as xa
    pair = scene["pair"]
    rng = np.random.default_rng(7)
    hi = pair.target.max(0)
    cluster = (np.array([hi[0] + 15.0, 0.0, 2.0]) + rng.uniform(-2.0, 2.0, (300, 3))).astype(np.float32)
    ang = rng.uniform(0, 2 * math.pi, 5)
    far = np.stack([330.0 * np.cos(ang), 330.0 * np.sin(ang), rng.uniform(-5, 5, 5)], 1).astype(np.float32)
    src = np.concatenate([scene["src_map"][:1500], cluster, far]).astype(np.float32)
    ref = R.icp(src, pair.target, tgt=scene["tgt"], max_iter=1)
    assert ref["history"][0]["pairs"] == len(src)
    with make_icp(xa, pair.target, src, max_iter=1) as icp:
        icp.align(want_output=False)
        check_first_iteration(icp, ref)
        # with the identity both kernels' queries are the source points themselves: getFitnessScore's minimum and the
        # pass's argmin come out of one walk (in-grid cells, cells outside the grid, block shells) bit for bit
        _, d_fit = icp.getFitnessScore(T=np.eye(4, dtype=np.float32), return_distances=True)
        assert np.array_equal(d_fit.view(np.uint32), icp.correspondences()[1].view(np.uint32))
    # the same with pgo_node's 150 m: the 5 far points are searched (their d2 is reported) and rejected
    ref = R.icp(src, pair.target, tgt=scene["tgt"], max_iter=1, max_corr_dist=150.0)
    assert ref["history"][0]["pairs"] == len(src) - 5
    with make_icp(xa, pair.target, src, max_iter=1, max_corr_dist=150.0) as icp:
        icp.align(want_output=False)
        check_first_iteration(icp, ref)


@pytest.mark.parametrize("n_source", [3, 17, 64, 65, 4097])
def test_sizes(scene, n_source):
    """The fewest points an estimate takes, a partial wave of teams, 64 and 65 queries (four and four-plus workgroup
    steps), and 4097 = 257 workgroups: the tail's threads sum more than one group of partials."""
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["src_map"][:n_source]
    ref = R.icp(src, pair.target, tgt=scene["tgt"], max_iter=1)
    with make_icp(xa, pair.target, src, max_iter=1) as icp:
        out = icp.align()
        dev = check_first_iteration(icp, ref)
        assert dev[0]["pairs"] == n_source
        assert np.max(np.abs(dev[0]["T"] - ref["history"][0]["T"])) < TF_TOL
        assert np.max(np.abs(icp.getFinalTransformation() - ref["final"])) < TF_TOL
        assert out.shape == (n_source, 3)
        assert np.array_equal(out, R.transform_f32(icp.getFinalTransformation(), src))


def test_two_points_is_no_correspondences(scene):
    import xchu_slam_amd as xa
    pair = scene["pair"]
    with make_icp(xa, pair.target, pair.source[:2]) as icp:
        icp.align(scene["guess"], want_output=False)
        r = icp.result()
        assert (r["state"], r["converged"], r["nr_iterations"], r["n_pairs"]) == (R.NO_CORRESPONDENCES, False, 0, 2)
        assert np.array_equal(r["final_tf"], scene["guess"])


# worst |T_device - T_restatement| over every incremental and final transform of the two cases, as measured on the
# MI355X: recorded in DESIGN.md (ICP section)
@pytest.mark.parametrize("prm", [PGO, dict(max_iter=10, trans_eps=0.0, fit_eps=0.0)], ids=["pgo_node", "ten_iterations"])
def test_full_align(scene, prm):
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["src_map"][:3000]
    ref = R.icp(src, pair.target, tgt=scene["tgt"], **prm)
    with make_icp(xa, pair.target, src, **prm) as icp:
        icp.align(want_output=False)
        r, dev = icp.result(), icp.history()
        print("iterations", r["nr_iterations"], "state", R.STATE_NAMES[r["state"]], "restatement", ref["iterations"],
              R.STATE_NAMES[ref["state"]])
        assert (r["nr_iterations"], r["state"], r["converged"]) == (ref["iterations"], ref["state"], ref["converged"])
        assert [h["pairs"] for h in dev] == [h["pairs"] for h in ref["history"]]
        assert [h["state"] for h in dev] == [h["state"] for h in ref["history"]]
        worst = max(float(np.max(np.abs(a["T"] - b["T"]))) for a, b in zip(dev, ref["history"]))
        worst = max(worst, float(np.max(np.abs(r["final_tf"] - ref["final"]))))
        print("worst |T - T_restatement|", worst)
        assert np.max(np.abs(r["final_tf"])) < 2.0  # the premise of the bar: one f32 ulp is at most 2.4e-7
        assert worst < TF_TOL
        print("mse", r["mse"], "restatement", ref["mse"])
        if prm is PGO:
            # known answer: guess then correction = the pair's true pose, within the smoke test's bounds
            t_err, r_err = pose_err(r["final_tf"].astype(np.float64) @ scene["guess"].astype(np.float64), pair.true_pose)
            print("pose error", t_err, "m", r_err, "deg")
            assert t_err < 0.2 and r_err < 0.5, (t_err, r_err)


def hist_bytes(h):
    return [(x["T"].tobytes(), x["pairs"], x["mse"], x["state"]) for x in h]


def test_deterministic(scene):
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["pair"].source[:3000]
    runs = []
    with make_icp(xa, pair.target, src, **PGO) as icp:
        for _ in range(2):
            icp.align(scene["guess"], want_output=False)
            runs.append((hist_bytes(icp.history()), icp.getFinalTransformation().tobytes()))
    with make_icp(xa, pair.target, src, **PGO) as icp:
        icp.align(scene["guess"], want_output=False)
        runs.append((hist_bytes(icp.history()), icp.getFinalTransformation().tobytes()))
    assert len(runs[0][0]) > 2
    assert runs[0] == runs[1] == runs[2]


def test_fitness_score_after_icp(scene):
    """getFitnessScore after an ICP align (T = None: the ICP's final transformation) is the value an NDT-only context
    gives for that transformation, bit for bit, distances included."""
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["pair"].source[:3000]
    with make_icp(xa, pair.target, src, **PGO) as icp:
        icp.align(scene["guess"], want_output=False)
        T = icp.getFinalTransformation()
        s_icp, d_icp = icp.getFitnessScore(return_distances=True)
        s_cap = icp.getFitnessScore(max_range=1.0)
    with xa.NormalDistributionsTransform() as ndt:
        ndt.setResolution(1.0)
        ndt.setInputTarget(pair.target)
        ndt.setInputSource(src)
        s_ndt, d_ndt = ndt.getFitnessScore(T=T, return_distances=True)
        s_ndt_cap = ndt.getFitnessScore(max_range=1.0, T=T)
    assert s_icp == s_ndt and s_cap == s_ndt_cap
    assert np.array_equal(d_icp.view(np.uint32), d_ndt.view(np.uint32))
    ref = R.fitness_score(src, pair.target, T, tgt=scene["tgt"])
    assert abs(s_icp - ref) <= 1e-12 * ref


def test_ndt_align_after_icp(scene):
    """An NDT align on a context that has run ICP (and carries the index's fifth word) is bitwise a fresh context's."""
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["pair"].source[:3000]

    def ndt_run(with_icp):
        with xa.NormalDistributionsTransform() as ndt:
            ndt.setResolution(1.0)
            ndt.setStepSize(0.1)
            ndt.setTransformationEpsilon(0.01)
            ndt.setMaximumIterations(30)
            ndt.setInputTarget(pair.target)
            ndt.setInputSource(src)
            if with_icp:
                icp = xa.IterativeClosestPoint(registration=ndt)
                configure(icp, **PGO)
                icp.align(scene["guess"], want_output=False)
                assert icp.getFinalNumIteration() > 1
            out = ndt.align(pair.guess)
            fit = ndt.getFitnessScore()  # the NDT align's transformation again, not the ICP's
            hist = [(h["kind"], h["x"].tobytes(), h["score"], h["pairs"]) for h in ndt.history()]
            return ndt.getFinalTransformation().tobytes(), ndt.getFinalNumIteration(), hist, out.tobytes(), fit

    assert ndt_run(True) == ndt_run(False)


# ---------------------------------------------------------------------------------------------- refine_loop
def loop_keyframes(false_candidate=False):
    """12 keyframes of 1.5 k points cut from one scene (a dense map cloud; every keyframe is a random 1.5 k-point
    subsample of the map within 8 m of its position, in its sensor frame) along an out-and-back loop: 2 m steps out
    along x, turned around, the same way back, so keyframe 11 revisits keyframe 0's place and the target submap
    (keyframes 0..2) covers what it sees.  Odometry drift grows to 0.4 m at the last keyframe.  Returns the keyframes,
    their drifted poses and keyframe 11's true position.
    false_candidate: the last keyframe is cut at the far end of the scene while its pose claims the loop position."""
    from xchu_slam_amd import synth
    world = synth.make_world(3, half=40.0)
    cloud = world.target(6.0, 77).astype(np.float64)
    b = world.buildings
    start = b[np.argmin(np.hypot(b[:, 0] + 15, b[:, 1] + 15)), :2]
    other = b[np.argmax(np.hypot(b[:, 0] - start[0], b[:, 1] - start[1])), :2]
    rng = np.random.default_rng(9)
    keyframes, poses = [], []
    for i in range(12):
        back = i >= 6
        true = (start[0] + 2.0 * ((11 - i) if back else i), start[1] + 0.3 * i / 11, 1.73, 0.0, 0.0,
                (math.pi - 0.1) if back else 0.05)
        at = (other[0], other[1]) + true[2:] if (false_candidate and i == 11) else true
        near = cloud[np.hypot(cloud[:, 0] - at[0], cloud[:, 1] - at[1]) < 8.0]
        near = near[rng.permutation(len(near))[:1500]]
        inv = np.linalg.inv(synth.pose_matrix(*at))
        pts = (near @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        keyframes.append(np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(np.float32)], 1))
        drift = 0.4 * i / 11
        poses.append((true[0] + drift * 0.8, true[1] - drift * 0.6, true[2], 0.0, 0.0, true[5]))
    return keyframes, poses, np.array(true[:3])


def host_submap(xa, keyframes, poses, idxs, leaf):
    parts = []
    for i in idxs:
        T = R.get_transformation(*poses[i])
        parts.append(np.concatenate([R.transform_f32(T, keyframes[i][:, :3]), keyframes[i][:, 3:4]], 1))
    return xa.voxel_downsample(np.concatenate(parts).astype(np.float32), leaf)


def test_refine_loop():
    import xchu_slam_amd as xa
    from xchu_slam_amd.icp import get_transformation
    keyframes, poses, true11 = loop_keyframes()
    assert all(len(k) == 1500 for k in keyframes)
    assert np.array_equal(get_transformation(*poses[11]), R.get_transformation(*poses[11]))
    out = xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, return_clouds=True)
    # the submaps: keyframe 11 alone; keyframes 0..2 (the range clipped at 0)
    src = host_submap(xa, keyframes, poses, [11], 0.5)
    tgt = host_submap(xa, keyframes, poses, [0, 1, 2], 0.5)
    assert (out["n_source"], out["n_target"]) == (len(src), len(tgt))
    assert np.array_equal(out["source_cloud"].view(np.uint32), src.view(np.uint32))
    assert np.array_equal(out["target_cloud"].view(np.uint32), tgt.view(np.uint32))
    ref = R.icp(src, tgt, **PGO)
    print("iterations", out["iterations"], "restatement", ref["iterations"], "score", out["score"])
    assert (out["iterations"], out["state"], out["converged"]) == (ref["iterations"], ref["state"], ref["converged"])
    assert [h["pairs"] for h in out["history"]] == [h["pairs"] for h in ref["history"]]
    assert np.max(np.abs(out["transform"] - ref["final"])) < TF_TOL
    score = R.fitness_score(src, tgt, out["transform"])
    assert abs(out["score"] - score) <= 1e-12 * score
    assert out["accepted"] == (bool(ref["converged"]) and score <= float(np.float32(0.3))) and out["accepted"]
    # the correction takes keyframe 11 from its drifted pose (0.4 m off) back to its true place, up to the 0.07 m of
    # drift the target's own keyframes carry and the sampling noise
    corrected = out["transform"].astype(np.float64) @ R.get_transformation(*poses[11]).astype(np.float64)
    assert np.linalg.norm(np.array(poses[11][:3]) - true11) > 0.39
    assert np.linalg.norm(corrected[:3, 3] - true11) < 0.15


def test_refine_loop_rejects_a_false_candidate():
    import xchu_slam_amd as xa
    keyframes, poses, _ = loop_keyframes(false_candidate=True)
    out = xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, return_clouds=True)
    score = R.fitness_score(out["source_cloud"], out["target_cloud"], out["transform"])
    assert abs(out["score"] - score) <= 1e-12 * score
    assert score > 0.3 and not out["accepted"]


def test_refine_loop_literal_root():
    """literal_root reproduces the reference's LoopFindNearKeyframesCloud, which never reads `key`: the source is the loop
    keyframe itself, already inside the target submap."""
    import xchu_slam_amd as xa
    keyframes, poses, _ = loop_keyframes()
    out = xa.refine_loop(keyframes, poses, loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, literal_root=True,
                         return_clouds=True)
    assert np.array_equal(out["source_cloud"], host_submap(xa, keyframes, poses, [0], 0.5))
    assert out["accepted"] and np.max(np.abs(out["transform"] - np.eye(4))) < 0.05
