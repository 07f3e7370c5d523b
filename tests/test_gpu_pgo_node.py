"""pgo_node's Run loop on the device (xa.PGO, xa.run_mapping, PoseGraph.set_estimate) on the 102-keyframe loop route of
the Scan Context tests (sc_scene.route_keyframes(4200), bin-sensitive points removed, a random intensity column, as
test_close_loops has it): stamps 0.5 s apart, keyframe_gap 1.0 so that every scan is a keyframe, dist_thres 0.4 and
period 1 for the detector.  Two odometries: the truth perturbed as in test_close_loops, and pgo_scene.drifted_route's.

Every device step of the loop is an existing launch, so the loop is compared with those launches called by hand: bit
for bit where the same call is made on the same input, and for the final poses under the bound tests/test_gpu_pgo.py
uses: ten times the restatement's own spread on the graph, measured as that file measures it (tests/pgo_restate.py on the
CPU, sparse normal equations, step_eps 1e-10 against 1e-12, on the 102 nodes and the 24 loop factors each route's online
run logged): 5.23e-12 on the perturbed route (14 against 16 iterations), 4.72e-11 on the drifted one (33 against 39).
A reweighted iteration stopped at step_eps is a few step_eps from the stationary point, from whichever estimate it
started; that distance is the spread.  (test_gpu_pgo.py's own drifted route, with 12 loops built from the truth, has
1.52e-10.)
"""
import os

import numpy as np
import pytest

import isc_restate
import pgo_node_restate as R0
import pgo_scene
import sc_restate as SR
import sc_scene

pytestmark = pytest.mark.gpu

N = 102
DT = 0.5
DETECT = dict(dist_thres=0.4, tree_making_period=1)
REFINE = dict(search_num=25, leaf=0.5)
SPREAD = {"perturbed": 5.23e-12, "drifted": 4.72e-11, "chain": 1.14e-11}   # chain: test_gpu_pgo.py's small graphs
MAX_ITER, STEP_EPS = 5000, 1e-12
VARIANTS = ("perturbed", "drifted")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Run:
    """One replay of the route through xa.PGO, keyframe by keyframe, with what can only be seen while it runs: after every
    push whether `poses` is the odometry bit for bit, the optimise launches so far and the length of the graph's history;
    and for every refined record the same refine_loop call made by hand on the record's poses_before."""

    def __init__(self, keyframes, odom, **kw):
        import xchu_slam_amd as xa
        self.odom = np.asarray(odom, np.float64)
        self.times = DT * np.arange(len(keyframes))
        # The bound is for estimates at their stationary point.  With one or two loops against 100 odometry edges the
        # reweighted iteration of the drifted route contracts slowly (319 steps to 1e-10): cut off at the default 200
        # steps, or stopped at the default step_eps with a rate near 1, such an intermediate estimate is further from
        # its stationary point than the final graph's spread, and the next ICP sees it.  So every solve here runs to 1e-12.
        args = dict(REFINE, keyframe_gap=1.0, detect_args=DETECT, pgo_args=dict(max_iter=MAX_ITER, step_eps=STEP_EPS))
        args.update(kw)
        if args.get("loop_method", 1) == 0:
            args["detect_args"] = None
        self.pgo = xa.PGO(**args)
        self.is_odometry, self.launches, self.history_len, self.by_hand = [], [], [], {}
        refine = dict(REFINE, score_threshold=kw.get("score_threshold", 0.3))
        for k, (cloud, pose) in enumerate(zip(keyframes, self.odom)):
            rec = self.pgo.push(cloud, pose, self.times[k])
            assert rec["keyframe"] and rec["index"] == k and len(rec["poses_before"]) == k + 1
            self.is_odometry.append(same_bits(self.pgo.poses, self.odom[:k + 1]))
            self.launches.append(self.pgo.optimize_launches)
            self.history_len.append(len(self.pgo.graph.history()))
            if rec["refined"]:
                self.by_hand[k] = xa.refine_loop(None, rec["poses_before"], rec["candidate"], k, store=self.pgo.store, **refine)
        self.log = self.pgo.log
        self.accepted = [r for r in self.log if r["accepted"]]
        self.refined = [r for r in self.log if r["refined"]]
        self.solves = [r["info"] for r in self.log if r["info"]]


@pytest.fixture(scope="module")
def scene():
    scans, truth = sc_scene.route_keyframes(4200)
    assert len(scans) == N
    scans = [np.delete(s, SR.bin_sensitive(s), axis=0) for s in scans]
    rng = np.random.default_rng(17)
    keyframes = [np.concatenate([s, rng.uniform(0, 1, (len(s), 1)).astype(np.float32)], 1) for s in scans]
    amp = np.array([0.3, 0.3, 0.05, np.radians(0.5), np.radians(0.5), np.radians(1.0)])
    perturbed = np.array([np.array(p) + rng.uniform(-1, 1, 6) * amp for p in truth])
    from xchu_slam_amd.posegraph import _matrix_to_pose6d
    drifted = np.array([_matrix_to_pose6d(T) for T in pgo_scene.drifted_route(truth)[1]])
    detections = SR.detect_loops([SR.make_scancontext(s) for s in scans], **DETECT)
    assert not any(r["tie"] for r in detections)
    sc = {"keyframes": keyframes, "truth": np.array(truth), "odom": {"perturbed": perturbed, "drifted": drifted},
          "detections": [r["loop_id"] for r in detections], "runs": {}}
    yield sc
    for run in sc["runs"].values():
        run.pgo.close()


def replay(scene, variant, **kw):
    key = (variant, repr(sorted(kw.items())))
    if key not in scene["runs"]:
        scene["runs"][key] = Run(scene["keyframes"], scene["odom"][variant], **kw)
    return scene["runs"][key]


# ---------------------------------------------------------------------------------------------- the loop, method 1
@pytest.mark.parametrize("variant", VARIANTS)
def test_candidates_are_the_detections(scene, variant):
    """From keyframe 30 on the candidates are sc_restate.detect_loops' detections; none before."""
    run = replay(scene, variant)
    want = scene["detections"]
    assert sum(1 for v in want if v != -1) >= 15 and all(v == -1 for v in want[:30])
    assert [r["candidate"] for r in run.log] == want
    assert all(r["gate"] == "too_few" for r in run.log[:29]) and run.log[29]["gate"] == "none"
    for r in run.log[29:]:             # a revisit is within a few metres of its match on both odometries
        assert r["gate"] == ("none" if r["candidate"] == -1 else "ok") and r["refined"] == (r["candidate"] != -1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_refined_records_are_refine_loop_bitwise(scene, variant):
    run = replay(scene, variant)
    assert len(run.refined) >= 15 and len(run.accepted) >= 1
    for r in run.refined:
        one = run.by_hand[r["index"]]
        assert same_bits(one["transform"], r["transform"]) and one["transform"].dtype == np.float32, r["index"]
        assert one["score"] == r["score"] and one["accepted"] == r["accepted"], r["index"]
    assert [(a, b) for a, b, *_ in run.pgo.loops] == [(r["candidate"], r["index"]) for r in run.accepted]
    assert [(a, b) for a, b, why in run.pgo.rejected if why == "icp"] == [(r["candidate"], r["index"]) for r in run.refined if not r["accepted"]]
    for (a, b, T, s), r in zip(run.pgo.loops, run.accepted):
        assert same_bits(T, r["transform"]) and s == r["score"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_before_the_first_accepted_loop(scene, variant):
    """No launch of the solver and `poses` is the odometry bit for bit; the first accepted loop is close_loops' entry for
    that pair bit for bit (both work on the odometry there)."""
    import xchu_slam_amd as xa
    run = replay(scene, variant)
    first = run.accepted[0]["index"]
    assert first >= 30
    assert all(run.is_odometry[:first]) and not run.is_odometry[first]
    assert run.launches[:first] == [0] * first and run.launches[first] == 1
    assert run.history_len[:first] == [0] * first and run.history_len[first] >= 1
    assert all(not r["optimized"] and r["info"] is None for r in run.log[:first]) and run.log[first]["optimized"]
    assert same_bits(run.log[first]["poses_before"], run.odom[:first + 1])
    accepted, rejected = xa.close_loops(scene["keyframes"], [tuple(p) for p in run.odom], detect_args=DETECT, store=run.pgo.store, **REFINE)
    entry = [a for a in accepted if (a[0], a[1]) == (run.accepted[0]["candidate"], first)]
    assert len(entry) == 1
    assert same_bits(entry[0][2], run.accepted[0]["transform"]) and entry[0][3] == run.accepted[0]["score"]
    # whatever close_loops refined before it, the online loop refined too, with the same outcome
    for a, b, why in rejected:
        if b < first:
            assert why == "icp" and not run.log[b]["accepted"] and run.log[b]["refined"] and run.log[b]["candidate"] == a


@pytest.mark.parametrize("variant", VARIANTS)
def test_after_the_first_accepted_loop_the_corrected_poses_are_used(scene, variant):
    import xchu_slam_amd as xa
    run = replay(scene, variant)
    first = run.accepted[0]["index"]
    nxt = next(r for r in run.refined if r["index"] > first)
    k = nxt["index"]
    assert not same_bits(nxt["poses_before"], run.odom[:k + 1])
    assert np.abs(nxt["poses_before"] - run.odom[:k + 1]).max() > 1e-6
    on_odom = xa.refine_loop(None, run.odom, nxt["candidate"], k, store=run.pgo.store, **REFINE)
    assert not same_bits(on_odom["transform"], nxt["transform"])


def by_hand_graph(xa, run):
    pg = xa.PoseGraph(max_iter=MAX_ITER, step_eps=STEP_EPS)
    for p in run.odom:
        pg.add_node(p)
    for r in run.accepted:
        pg.add_loop(r["candidate"], r["index"], r["measurement"], r["score"], 1.0)
    return pg


@pytest.mark.parametrize("variant", VARIANTS)
def test_final_poses(scene, variant):
    """The online estimate against one optimise of the same graph built by hand, and `append="predict"` against
    `append="optimize"`: the two runs end to end, the literal sequence of solves (one after every node and one after every
    loop factor) made by hand on the factors the "predict" run logged, and the "optimize" run against the by-hand graph of
    its own factors, all under the bound.  Every solve must have converged (see Run)."""
    import xchu_slam_amd as xa
    TOL = 10 * SPREAD[variant]
    run = replay(scene, variant)
    X = run.pgo.graph.poses()
    assert np.all(np.isfinite(X)) and len(run.pgo.poses) == N
    other = replay(scene, variant, append="optimize")
    assert all(i["converged"] for i in run.solves) and all(i["converged"] for i in other.solves)
    assert run.launches[-1] == run.pgo.optimize_launches == len(run.accepted)       # one solve per accepted loop
    with by_hand_graph(xa, run) as pg:
        info = pg.optimize()
        Xh, P6 = pg.poses(), pg.poses6d()
    assert info["converged"]
    d_hand = np.abs(X - Xh).max()
    d6 = run.pgo.poses - P6
    d6[:, 3:] = (d6[:, 3:] + np.pi) % (2 * np.pi) - np.pi
    # the reference's literal sequence on the same factors: a solve after every node and after every loop factor
    loops = {r["index"]: r for r in run.accepted}
    solves = 0
    with xa.PoseGraph(max_iter=MAX_ITER, step_eps=STEP_EPS) as pg:
        for k, p in enumerate(run.odom):
            pg.add_node(p)
            assert pg.optimize()["converged"]
            solves += 1
            if k in loops:
                r = loops[k]
                pg.add_loop(r["candidate"], k, r["measurement"], r["score"], 1.0)
                assert pg.optimize()["converged"]
                solves += 1
        Xl = pg.poses()
    d_literal = np.abs(X - Xl).max()
    # append="optimize" end to end: the same check against the graph of its own logged factors
    Xo = other.pgo.graph.poses()
    with by_hand_graph(xa, other) as pg:
        assert pg.optimize()["converged"]
        d_hand_o = np.abs(Xo - pg.poses()).max()
    same = [(a, b) for a, b in zip(run.accepted, other.accepted) if (a["candidate"], a["index"]) == (b["candidate"], b["index"])]
    d_factor = max(np.abs(a["measurement"] - b["measurement"]).max() for a, b in same)
    d_before = max(np.abs(a["poses_before"] - b["poses_before"]).max() for a, b in same)
    d_runs = np.abs(X - Xo).max()
    moved = np.abs(run.pgo.poses[:, :3] - run.odom[:, :3]).max()
    print(f"{variant}: loops {len(run.accepted)} |online - by hand| {d_hand:.3e} |poses6d| {np.abs(d6).max():.3e} "
          f"|predict - literal sequence, same factors| {d_literal:.3e} ({solves} solves) |optimize run - its by hand| {d_hand_o:.3e} "
          f"|predict run - optimize run| {d_runs:.3e} with |poses_before| {d_before:.3e} |Z| {d_factor:.3e} between the runs "
          f"(launches {run.pgo.optimize_launches} / {other.pgo.optimize_launches}, CG {run.pgo.cg_iterations} / {other.pgo.cg_iterations}) "
          f"moved {moved:.3f} m, tol {TOL:.3e}")
    assert moved > 0.01
    assert d_hand <= TOL and np.abs(d6).max() <= 2 * TOL
    assert d_literal <= TOL                                        # "predict" against "optimize" on the same factors
    assert d_hand_o <= TOL
    assert other.pgo.optimize_launches == N + len(other.accepted)
    assert [(r["candidate"], r["index"], r["accepted"]) for r in other.refined] == [(r["candidate"], r["index"], r["accepted"]) for r in run.refined]
    assert len(same) == len(run.accepted) and d_before <= TOL      # the two runs hand ICP the same poses within the bound
    assert d_runs <= TOL                                           # and end where the other ends


def test_literal_reject_stops(scene):
    """With the score threshold at the median score of the default run's loops some loops are rejected and some accepted
    (the early revisits score worst here): the default goes on refining after a rejection and accepts later loops,
    literal_reject_stops refines nothing after the first rejection."""
    base = replay(scene, "perturbed")
    thr = float(np.median([r["score"] for r in base.refined]))
    on = replay(scene, "perturbed", score_threshold=thr)
    stop = replay(scene, "perturbed", score_threshold=thr, literal_reject_stops=True)
    rejected = [r["index"] for r in on.refined if not r["accepted"]]
    assert rejected, "input condition: a loop scores above the threshold"
    r0 = rejected[0]
    assert any(r["index"] > r0 and r["accepted"] for r in on.refined), "input condition: a later loop is accepted"
    for a, b in zip(on.log[:r0 + 1], stop.log[:r0 + 1]):
        assert (a["candidate"], a["gate"], a["refined"], a["accepted"], a["score"]) == (b["candidate"], b["gate"], b["refined"], b["accepted"], b["score"])
    assert stop.log[r0]["refined"] and not stop.log[r0]["accepted"]
    assert not any(r["refined"] for r in stop.log[r0 + 1:])
    later = [r for r in stop.log[r0 + 1:] if r["candidate"] != -1]
    assert later and all(r["gate"] == "ok" and not r["accepted"] and r["transform"] is None for r in later)   # detection goes on
    assert [r["candidate"] for r in stop.log] == scene["detections"]
    assert stop.pgo.optimize_launches == len(stop.accepted) == sum(1 for r in on.log[:r0] if r["accepted"])
    assert len(on.accepted) > len(stop.accepted)


# ---------------------------------------------------------------------------------------------- methods 0 and 2
def test_loop_method_0(scene):
    """Revisits are 79 keyframes, 39.5 s, later.  The candidates are the host restatement's on the logged poses_before and
    times; the gate is its distance test."""
    run = replay(scene, "perturbed", loop_method=0)
    assert run.pgo.detector is None
    found = 0
    for r in run.log:
        k = r["index"]
        want = R0.radius_candidate(r["poses_before"], run.times[:k + 1])
        assert r["candidate"] == want, (k, r["candidate"], want)
        if want == -1:
            assert r["gate"] == ("too_few" if k < 29 else "none") and not r["refined"]
            continue
        found += 1
        assert run.times[k] - run.times[want] > 30.0
        assert R0.radius_accept(r["poses_before"], want, k) and r["gate"] == "ok" and r["refined"]
        one = run.by_hand[k]
        assert same_bits(one["transform"], r["transform"]) and one["score"] == r["score"] and one["accepted"] == r["accepted"]
    assert found >= 15 and all(r["candidate"] == -1 for r in run.log[:61])     # nothing is 30 s old before keyframe 61
    assert abs(run.log[N - 1]["candidate"] - (N - 1 - 79)) <= 3
    assert np.all(np.isfinite(run.pgo.poses)) and run.pgo.optimize_launches == len(run.accepted)


def test_loop_method_2(scene):
    """The candidates are isc_restate's detections on the same keyframes at the odometry's (x, y, 0)."""
    run = replay(scene, "perturbed", loop_method=2, detect_args={})
    g = isc_restate.ISCGeneration()
    want = []
    for cloud, p in zip(scene["keyframes"], run.odom):
        g.makeAndSavedec(cloud, (p[0], p[1], 0.0))
        want.append(g.detectLoopClosureID()[0])
    got = [r["candidate"] for r in run.log]
    assert all(c == -1 for c in got[:29]) and got[29:] == want[29:]
    assert run.pgo.detector.shape == (60, 60) and len(run.pgo.detector) == N
    for r in run.refined:
        one = run.by_hand[r["index"]]
        assert same_bits(one["transform"], r["transform"]) and one["score"] == r["score"]
    assert np.all(np.isfinite(run.pgo.poses))


def test_descriptors_from_the_store_pointer(scene):
    """The detectors' descriptors, made from the store's device pointer, are those of the host add bit for bit."""
    import xchu_slam_amd as xa
    sc_run = replay(scene, "perturbed")
    isc_run = replay(scene, "perturbed", loop_method=2, detect_args={})
    picks = [0, 1, 50, N - 1]
    with xa.SCManager(**DETECT) as sc, xa.ISCGeneration() as isc:
        for j, i in enumerate(picks):
            cloud = scene["keyframes"][i]
            assert np.array_equal(sc_run.pgo.store.keyframe(i), cloud)
            assert sc.makeAndSaveScancontextAndKeys(cloud) == j
            assert same_bits(sc.polarcontext(j), sc_run.pgo.detector.polarcontext(i))
            assert same_bits(sc.ringkey(j), sc_run.pgo.detector.ringkey(i))
            assert same_bits(sc.sectorkey(j), sc_run.pgo.detector.sectorkey(i))
            p = isc_run.odom[i]
            assert isc.makeAndSavedec(cloud, (p[0], p[1], 0.0)) == j
            assert np.array_equal(isc.descriptor(j), isc_run.pgo.detector.descriptor(i))
            assert same_bits(isc.position(j)[0], isc_run.pgo.detector.position(i)[0])
            assert isc_run.pgo.detector.position(i)[0][2] == 0.0


# ---------------------------------------------------------------------------------------------- GPS, set_estimate
def test_gps_altitude_factors(scene):
    """useGPS on the first 40 keyframes: no factor on node 0, the offset is the first keyframe's altitude, x and y come from
    the last optimised pose; a node with a position factor is solved for, a node without one is predicted."""
    import xchu_slam_amd as xa
    odom = scene["odom"]["perturbed"][:40]
    alt = 100.0 + scene["truth"][:40, 2] + 0.5 * np.sin(np.arange(40))
    fixes = {k: alt[k] for k in range(40) if k % 3 != 1}
    with xa.PGO(keyframe_gap=1.0, detect_args=DETECT, **REFINE) as pgo:
        for k in range(40):
            before = pgo.poses.copy()
            rec = pgo.push(scene["keyframes"][k], odom[k], DT * k, fixes.get(k))
            if k == 0 or k not in fixes:
                assert rec["gps"] is None and not rec["optimized"]
            else:
                assert rec["optimized"] and same_bits(rec["gps"], np.array([before[k - 1, 0], before[k - 1, 1], alt[k] - alt[0]]))
        n_fix = len(fixes) - 1
        assert pgo.optimize_launches == n_fix and len(pgo.graph.position_weights()) == n_fix
        X = pgo.graph.poses()
        with xa.PoseGraph() as pg:
            for p in odom:
                pg.add_node(p)
            for r in pgo.log:
                if r["gps"] is not None:
                    pg.add_position(r["index"], r["gps"], (1e9, 1e9, 250.0), 1.0)
            assert pg.optimize()["converged"]
            d = np.abs(pg.poses() - X).max()
        print(f"gps: |online - by hand| {d:.3e}")
        assert d <= 10 * SPREAD["chain"] and np.abs(pgo.poses[:, 2] - odom[:, 2]).max() > 1e-7


def test_set_estimate():
    """Host state only: the node's estimate is the pose given, bit for bit, nothing else moves, the factors are what they
    were (the next optimise returns to the same optimum); the validity rules are add_node's."""
    import xchu_slam_amd as xa
    from xchu_slam_amd._lib import NDT_EINVAL, NdtError
    true, est, loops = pgo_scene.circle(24, loop_every=3, max_loops=4)
    with xa.PoseGraph() as pg:
        for P in est:
            pg.add_node(P)
        for i, j, Z, var, k in loops:
            pg.add_loop(i, j, Z, var, k)
        pg.optimize()
        X = pg.poses()
        pg.set_estimate(7, true[7])
        Y = pg.poses()
        assert same_bits(Y[7], true[7]) and same_bits(np.delete(Y, 7, 0), np.delete(X, 7, 0)) and len(pg) == 24
        pg.set_estimate(23, xa.posegraph._matrix_to_pose6d(true[23]))      # a Pose6D is taken like add_node takes it
        info = pg.optimize()
        assert info["converged"] and np.abs(pg.poses() - X).max() <= 10 * 1.14e-11
        # a node appended with X_{k-1} (P_{k-1}^-1 P_k) leaves a stationary estimate stationary: one step below step_eps
        P_new = est[23] @ np.linalg.inv(est[22]) @ est[23]
        X = pg.poses()
        k = pg.add_node(P_new)
        pg.set_estimate(k, X[23] @ (np.linalg.inv(est[23]) @ P_new))
        info = pg.optimize()
        assert info["iterations"] == 1 and info["max_step"] < 1e-10 and np.abs(pg.poses()[:24] - X).max() <= 10 * 1.14e-11

        def bad(call, text):
            before = pg.poses()
            with pytest.raises(NdtError) as ei:
                call()
            assert ei.value.status == NDT_EINVAL and text in str(ei.value), str(ei.value)
            assert same_bits(pg.poses(), before)

        bad(lambda: pg.set_estimate(25, true[3]), "node index out of range")
        bad(lambda: pg.set_estimate(-1, true[3]), "node index out of range")
        bad(lambda: pg.set_estimate(3, 2.0 * true[3]), "finite rigid")
        nan = true[3].copy()
        nan[0, 3] = np.nan
        bad(lambda: pg.set_estimate(3, nan), "finite rigid")
        mirror = true[3].copy()
        mirror[:3, 0] = -mirror[:3, 0]
        bad(lambda: pg.set_estimate(3, mirror), "finite rigid")


# ---------------------------------------------------------------------------------------------- run_mapping
def test_run_mapping(scene, tmp_path):
    """filter_scan -> LidarOdom -> PGO on the first 60 poses of the route (3000-point scans), saved with SaveMap's files.
    Accuracy is recorded, not asserted."""
    import xchu_slam_amd as xa
    scans, truth = sc_scene.route_keyframes(3000)
    rng = np.random.default_rng(23)
    scans = [np.concatenate([s, rng.uniform(0, 1, (len(s), 1)).astype(np.float32)], 1) for s in scans[:60]]
    stamps = 100.0 + 0.1 * np.arange(60)
    out = tmp_path / "map"
    st = xa.run_mapping(scans, stamps, str(out), detect_args=DETECT)
    n = len(st["keyframes"])
    assert st["odometry"].shape == (60, 6) and np.all(np.isfinite(st["odometry"])) and np.all(np.isfinite(st["poses"]))
    assert st["keyframes"].tolist() == xa.keyframe_gate(st["odometry"]).tolist() and 2 <= n <= 60 and st["keyframes"][0] == 0
    assert same_bits(st["odom_poses"], st["odometry"][st["keyframes"]]) and same_bits(st["times"], stamps[st["keyframes"]])
    assert st["poses"].shape == (n, 6) and len(st["log"]) == n and np.all(np.isfinite(st["final_map"]))
    if not st["loops"]:
        assert same_bits(st["poses"], st["odom_poses"]) and st["optimize_launches"] == 0
    # the five files are the writers' output for the returned state, and read back to it
    assert sorted(os.listdir(out)) == ["finalMap.pcd", "lidar_odom.txt", "odom_tum.txt", "pose_graph.g2o", "trajectory.pcd"]
    want = tmp_path / "want"
    os.makedirs(want)
    traj = np.zeros((n, 4), np.float32)
    traj[:, :3] = st["poses"][:, :3]
    xa.write_pcd(want / "trajectory.pcd", traj)
    xa.write_pcd(want / "finalMap.pcd", st["final_map"])
    xa.write_tum(want / "odom_tum.txt", st["times"], st["poses"])
    xa.write_tum(want / "lidar_odom.txt", stamps, st["odometry"])
    xa.write_g2o(want / "pose_graph.g2o", st["poses"])
    for name in os.listdir(want):
        assert open(out / name, "rb").read() == open(want / name, "rb").read(), name
    assert len(xa.read_pcd(out / "finalMap.pcd")) == len(st["final_map"]) > 100
    assert np.allclose(xa.read_pcd(out / "trajectory.pcd")[:, :3], st["poses"][:, :3], rtol=1e-6, atol=1e-6)
    assert np.allclose(xa.read_g2o(out / "pose_graph.g2o")[:, :3], st["poses"][:, :3], rtol=1e-5, atol=1e-5)
    tum = np.loadtxt(out / "lidar_odom.txt")
    assert tum.shape == (60, 8) and np.allclose(tum[:, 0], stamps)
    # accuracy against the generating poses, recorded: the odometry starts at the origin, so the alignment is part of it
    from xchu_slam_amd.globalmap import VELO2CAMERA, matrix_to_quaternion
    from xchu_slam_amd.synth import pose_matrix
    ref = np.array([[t, *(VELO2CAMERA @ pose_matrix(*p))[:3, 3], *matrix_to_quaternion((VELO2CAMERA @ pose_matrix(*p))[:3, :3])]
                    for t, p in zip(stamps, truth[:60])])
    a, r = xa.ape(tum, ref), xa.rpe(tum, ref)
    print(f"run_mapping: {n} keyframes of 60 scans, loops {len(st['loops'])}, APE rmse {a['rmse']:.3f} m max {a['max']:.3f} m over "
          f"{a['path_length']:.1f} m, RPE rmse {r['rmse']:.3f} m")
    assert a["matched"] == 60


def test_push_refuses_before_any_state_moves(scene):
    """A cloud of the wrong shape, a non-finite pose or altitude: refused with the gate, the store, the detector and the
    graph where they were, so the next good scan gets the next index everywhere."""
    import xchu_slam_amd as xa
    odom, clouds = scene["odom"]["perturbed"], scene["keyframes"]
    with xa.PGO(keyframe_gap=1.0, detect_args=DETECT, **REFINE) as pgo:
        pgo.push(clouds[0], odom[0], 0.0)
        bad_pose = odom[1].copy()
        bad_pose[4] = np.nan
        for cloud, pose, alt in ((clouds[1][:, :3], odom[1], None), (clouds[1], bad_pose, None), (clouds[1], odom[1], np.inf),
                                 (clouds[1], odom[1][:5], None)):
            with pytest.raises(ValueError):
                pgo.push(cloud, pose, DT, alt)
            assert (len(pgo), len(pgo.store), len(pgo.detector), len(pgo.graph), pgo.scans, len(pgo.log)) == (1, 1, 1, 1, 1, 1)
        rec = pgo.push(clouds[1], odom[1], DT)
        assert rec["keyframe"] and rec["index"] == 1
        assert (len(pgo), len(pgo.store), len(pgo.detector), len(pgo.graph), pgo.scans) == (2, 2, 2, 2, 2)
        assert same_bits(pgo.poses, odom[:2])
        # the log can leave poses_before out of records that were not refined; push still returns it
        pgo.keep_poses_before = False
        rec = pgo.push(clouds[2], odom[2], 2 * DT)
        assert len(rec["poses_before"]) == 3 and pgo.log[2]["poses_before"] is None and pgo.log[1]["poses_before"] is not None
