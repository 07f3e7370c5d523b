"""The pose graph's direct loop-space solve on the device (xa.PoseGraph(solver="direct"), csrc/posegraph_direct.hip)
against tests/pgo_restate.py and tests/pgo_position_restate.py, on the graphs and with the acceptance and tolerances of
tests/test_gpu_pgo.py and tests/test_gpu_pgo_position.py (ten times the restatement's own spread per graph class on
poses, their weight bounds, the restatement's Gauss-Newton step at the device's poses below 10 step_eps, costs at 1e-9).
Every graph is also solved with conjugate gradients on the device: the two agree within twice the class tolerance (each
is within one of the restatement) and their iteration counts differ by at most one (a step just under or over step_eps
can fall either way).

Shapes: d = 6 loops + 3 positions is 0 (n = 1, n = 2, a chain), 24 (less than one 32-wide tile), 42, 96 (three whole
tiles), 102 (one factor more), 732 (the hub graph: a node in 71 loops), and odd with the position scenes (d = 24 on a
chain with a factor on node 0, 63, 27, 2292 on the hub graph)."""
import numpy as np
import pytest

import pgo_restate as R
import pgo_position_restate as PR
import pgo_position_scene as PS
import pgo_scene as S
import sc_scene
import test_gpu_pgo as G
import test_gpu_pgo_position as GP

pytestmark = pytest.mark.gpu

STEP_EPS = G.STEP_EPS
TILE = 32     # ndt::kPgoDirectTile
LIMIT = 8192  # ndt::kPgoDirectMaxDim


def device_graph(xa, est, loops, positions=(), **params):
    pg = xa.PoseGraph(**params)
    for P in est:
        pg.add_node(P)
    for i, j, Z, var, k in loops:
        pg.add_loop(i, j, Z, var, k)
    for node, xyz, var, k in positions:
        pg.add_position(node, xyz, var, k)
    return pg


def run(est, loops, positions=(), solver="direct"):
    import xchu_slam_amd as xa
    with device_graph(xa, est, loops, positions, solver=solver) as pg:
        assert pg.solver == solver
        info = pg.optimize()
        return dict(info=info, X=pg.poses(), w=pg.weights(), pw=pg.position_weights(), hist=pg.history(), stats=pg.solver_stats())


def check_direct(est, loops, positions, g, Xr, pose_tol, solver):
    """test_gpu_pgo.compare's acceptance for a DIRECT run, the solver's own invariants, and the CG run of the same graph."""
    out, cg = run(est, loops, positions, "direct"), run(est, loops, positions, "cg")
    info, X, hist, st = out["info"], out["X"], out["hist"], out["stats"]
    d = 6 * len(loops) + 3 * len(positions)
    assert st["solver"] == "direct" and st["d"] == d and st["tile"] == TILE and cg["stats"]["solver"] == "cg" and cg["stats"]["d"] == d
    assert st["factorizations"] == (info["iterations"] if d else 0)
    assert np.all(np.isfinite(X)) and np.all(X[:, 3] == [0, 0, 0, 1])
    assert info["converged"] and info["iterations"] == len(hist) >= 1
    assert info["cg_iterations"] == 0 and all(r["cg_iterations"] == 0 for r in hist)
    assert hist[0]["cost"] == info["cost0"] and hist[-1]["max_step"] == info["max_step"] < STEP_EPS
    step, worst, apart = np.abs(g.gn_step_at(X, solver)).max(), np.abs(X - Xr).max(), np.abs(X - cg["X"]).max()
    print(f"d {d}: iterations {info['iterations']} (CG {cg['info']['iterations']}), restatement's step at the device's poses "
          f"{step:.3e}, |X - Xr| {worst:.3e} (tolerance {pose_tol:.3e}), |X - X_cg| {apart:.3e}, refined {st['refined']}")
    assert step < 10 * STEP_EPS
    assert worst <= pose_tol, worst
    assert abs(info["cost"] - g.cost(X)) <= 1e-9 * max(1.0, info["cost"]) and abs(info["cost0"] - g.cost(est)) <= 1e-9 * max(1.0, info["cost0"])
    assert len(out["w"]) == len(loops) and len(out["pw"]) == len(positions)
    assert apart <= 2 * pose_tol and abs(info["iterations"] - cg["info"]["iterations"]) <= 1
    assert info["cost0"] == cg["info"]["cost0"]
    return out


_restated = {}


def restated(key, make, solver):
    """The restatement's optimum of a loops-only graph, computed once."""
    if key not in _restated:
        est, loops = make()
        g = R.build(est, loops)
        Xr, ir = g.optimize(solver=solver, step_eps=STEP_EPS)
        assert ir["converged"]
        Xr.setflags(write=False)
        _restated[key] = (est, loops, g, Xr)
    return _restated[key]


def loops_case(key, make, cls, solver="lstsq"):
    est, loops, g, Xr = restated(key, make, solver)
    out = check_direct(est, loops, (), g, Xr, G.tol(cls), solver)
    assert np.all(np.abs(out["w"] - g.weights(Xr)) <= G.weight_tol(g, Xr, cls))
    return out, g, Xr


def test_no_loops():
    """d = 0 (n = 1, n = 2, a 40-node chain): the step is y = g, nothing is built or factorised."""
    _, est, _ = S.circle(40)
    one = run(est[:1], [])
    assert one["info"]["converged"] and one["info"]["cost0"] == 0.0 == one["info"]["cost"] and one["info"]["max_step"] == 0.0
    assert np.array_equal(one["X"], est[:1]) and one["stats"] == dict(solver="direct", d=0, tile=TILE, factorizations=0, refined=False)
    for n in (2, 40):
        out, _, _ = loops_case(("chain", n), lambda: (est[:n], []), "circle")
        assert np.abs(out["X"] - est[:n]).max() < 1e-12 and out["info"]["iterations"] == 1


@pytest.mark.parametrize("n,kw,loops,d", [(24, dict(loop_every=3, max_loops=4), 4, 24), (65, {}, 7, 42),
                                          (65, dict(loop_every=2, max_loops=16), 16, 3 * TILE),
                                          (65, dict(loop_every=2), 17, 3 * TILE + 6)])
def test_circle(n, kw, loops, d):
    """Less than one tile; more than one; an exact multiple of the tile width; one factor more than that."""
    def make():
        _, est, lp = S.circle(n, **kw)
        return est, lp
    out, g, Xr = loops_case(("circle", n, loops), make, "circle")
    assert out["stats"]["d"] == d == 6 * loops and out["info"]["cost"] < out["info"]["cost0"]


def hub_graph():
    _, est, loops = S.hub(G.THREADS + 7)
    return est, loops


def test_hub_graph():
    """519 nodes, d = 732 (23 tiles), the hub node in 71 loops: the densest overlap pattern."""
    out, g, Xr = loops_case("hub", hub_graph, "hub", "sparse")
    assert out["stats"]["d"] == 732 and sum(1 for l in restated("hub", hub_graph, "sparse")[1] if 10 in l[:2]) >= 70


def test_reversed_gaussian_and_outlier_loops():
    """test_gpu_pgo's three variants of circle(65): loops given as (j, i), one Gaussian loop, one loop 10 m off."""
    def reverse():
        _, est, loops = S.circle(65)
        return est, [(j, i, R.inv_se3(Z), var, k) for i, j, Z, var, k in loops]

    def gaussian():
        _, est, loops = S.circle(65)
        loops[2] = loops[2][:4] + (0.0,)
        return est, loops

    def outlier():
        _, est, loops = S.circle(65)
        Z = loops[3][2].copy()
        Z[:3, 3] += [10.0, 0.0, 0.0]
        loops[3] = (loops[3][0], loops[3][1], Z) + loops[3][3:]
        return est, loops

    out, _, _ = loops_case("reversed", reverse, "circle")
    assert all(i > j for i, j, *_ in restated("reversed", reverse, "lstsq")[1])
    out, _, _ = loops_case("gaussian", gaussian, "circle")
    assert out["w"][2] == 1.0 and np.all(np.delete(out["w"], 2) < 1.0)
    out, _, _ = loops_case("outlier", outlier, "circle")
    assert out["w"][3] < 0.01 and np.all(out["w"][3] < np.delete(out["w"], 3))


@pytest.mark.parametrize("scene,cls,solver", [(PS.chain, "circle", "lstsq"), (PS.circle, "circle", "lstsq"), (PS.hub, "hub", "sparse"),
                                              (PS.tight, "tight", "lstsq"), (PS.gaussian, "circle", "lstsq"), (PS.outlier, "circle", "lstsq")],
                         ids=lambda v: getattr(v, "__name__", None))
def test_position_scenes(scene, cls, solver):
    """Every scene of tests/pgo_position_scene.py but the route, with test_gpu_pgo_position's tolerances: odd d, a factor
    on node 0, two on one node, 520 on the hub graph."""
    true, est, loops, pos, g, Xr = GP.restated(scene, solver)
    out = check_direct(est, loops, pos, g, Xr, GP.tol(cls), solver)
    assert out["stats"]["d"] == 6 * len(loops) + 3 * len(pos)
    assert np.all(np.abs(out["pw"] - g.position_weights(Xr)) <= GP.position_weight_tol(g, Xr, cls))
    assert np.all(np.abs(out["w"] - g.weights(Xr)) <= GP.between_weight_tol(g, Xr, cls))
    if scene is PS.gaussian:
        assert out["pw"][2] == 1.0


def test_optimize_loops_on_the_drifted_route():
    """xa.optimize_loops(..., solver="direct") on the drifted 102-keyframe route: the restatement's poses."""
    import xchu_slam_amd as xa
    true, est, accepted = S.drifted_route(sc_scene.route_poses())
    loops = [(i, j, xa.loop_measurement(est, i, j, T), np.full(6, s), 1.0) for i, j, T, s in accepted]
    g = R.build(est, loops)
    Xr, ir = g.optimize(solver="sparse", step_eps=STEP_EPS)
    assert ir["converged"]
    poses6d, info = xa.optimize_loops(est, accepted, solver="direct")
    _, info_cg = xa.optimize_loops(est, accepted)
    worst = np.abs(info["poses"] - Xr).max()
    print(f"route: iterations {info['iterations']} (CG {info_cg['iterations']}), |X - Xr| {worst:.3e} (tolerance {G.tol('route'):.3e})")
    assert info["converged"] and poses6d.shape == (len(est), 6) and info["cg_iterations"] == 0 and info_cg["cg_iterations"] > 0
    assert worst <= G.tol("route")
    assert np.abs(g.gn_step_at(info["poses"], "sparse")).max() < 10 * STEP_EPS
    assert abs(info["cost"] - g.cost(info["poses"])) <= 1e-9 * max(1.0, info["cost"])
    assert np.abs(info["poses"] - info_cg["poses"]).max() <= 2 * G.tol("route") and abs(info["iterations"] - info_cg["iterations"]) <= 1
    with pytest.raises(ValueError):
        xa.optimize_loops(est, accepted, solver="qr")


def test_solver_reaches_the_graph_of_pgo_and_run_mapping():
    """xa.PGO(solver="direct") on the 102-keyframe loop route with perturbed odometry (tests/test_gpu_pgo_node.py's): its
    graph solves directly (cg_iterations 0 in every solve of the log) and ends within twice the route's tolerance of the
    same run under CG; a "solver" entry of pgo_args wins over solver=; run_mapping hands solver= on (an unknown one is
    PoseGraph's ValueError)."""
    import xchu_slam_amd as xa
    import sc_restate as SR
    scans, truth = sc_scene.route_keyframes(4200)
    scans = [np.delete(sc, SR.bin_sensitive(sc), axis=0) for sc in scans]
    rng = np.random.default_rng(17)
    keyframes = [np.concatenate([sc, rng.uniform(0, 1, (len(sc), 1)).astype(np.float32)], 1) for sc in scans]
    amp = np.array([0.3, 0.3, 0.05, np.radians(0.5), np.radians(0.5), np.radians(1.0)])
    odom = np.array([np.array(p) + rng.uniform(-1, 1, 6) * amp for p in truth])
    args = dict(keyframe_gap=1.0, detect_args=dict(dist_thres=0.4, tree_making_period=1), search_num=25, leaf=0.5)
    out = {}
    for solver in ("direct", "cg"):
        with xa.PGO(solver=solver, **args) as pgo:
            assert pgo.graph.solver == solver
            for k, (cloud, pose) in enumerate(zip(keyframes, odom)):
                pgo.push(cloud, pose, 0.5 * k)
            solves = [r["info"] for r in pgo.log if r["info"]]
            assert len(solves) >= 1 and len(pgo.loops) >= 1 and all(i["converged"] for i in solves)
            assert pgo.graph.solver_stats()["solver"] == solver and pgo.graph.solver_stats()["d"] == 6 * len(pgo.loops)
            if solver == "direct":
                assert pgo.cg_iterations == 0 and all(i["cg_iterations"] == 0 for i in solves)
            else:
                assert pgo.cg_iterations > 0
            out[solver] = (np.array(pgo.poses), len(pgo.loops), len(solves))
    assert out["direct"][1:] == out["cg"][1:]
    apart = np.abs(out["direct"][0] - out["cg"][0]).max()
    print(f"online: {out['cg'][1]} loops, {out['cg'][2]} solves, |poses_direct - poses_cg| {apart:.3e}")
    assert apart <= 2 * G.tol("route")
    with xa.PGO(solver="direct", pgo_args=dict(solver="cg"), **args) as pgo:
        assert pgo.graph.solver == "cg"
    with xa.PGO(pgo_args=dict(solver="direct"), **args) as pgo:
        assert pgo.graph.solver == "direct"
    with pytest.raises(ValueError):
        xa.run_mapping([keyframes[0]], [0.0], solver="qr")


def test_warm_start():
    """test_gpu_pgo's warm start under DIRECT: ten nodes and two loops added after an optimise land on the optimum of
    one optimise of the whole graph, in fewer iterations."""
    import xchu_slam_amd as xa
    true, est, loops = S.circle(65)
    first = [l for l in loops if l[1] < 55]
    rest = [l for l in loops if l[1] >= 55]
    whole = run(est, loops)
    with device_graph(xa, est[:55], first, solver="direct") as pg:
        info1 = pg.optimize()
        assert info1["converged"] and pg.solver_stats()["d"] == 6 * len(first)
        for P in est[55:]:
            pg.add_node(P)
        for i, j, Z, var, k in rest:
            pg.add_loop(i, j, Z, var, k)
        info2 = pg.optimize()
        X2 = pg.poses()
        assert len(pg.weights()) == len(loops) and pg.solver_stats()["d"] == 6 * len(loops)
    assert info2["converged"] and info2["iterations"] < whole["info"]["iterations"]
    assert np.abs(X2 - whole["X"]).max() <= G.tol("circle")
    assert np.abs(R.build(est, loops).gn_step_at(X2, "lstsq")).max() < 10 * STEP_EPS


def test_determinism():
    """Two DIRECT runs give bitwise equal poses, weights and records (the hub graph with a position factor per node)."""
    true, est, loops, pos = PS.hub()
    a, b = run(est, loops, pos), run(est, loops, pos)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("X", "w", "pw")) and a["info"] == b["info"] and a["hist"] == b["hist"]


def test_switching_solvers_on_a_live_graph():
    """CG -> DIRECT -> CG on one graph (more nodes and a loop before each call): the last call gives the bits a CG-only
    graph gives for the same sequence when its middle call's estimate is the same, so the middle estimate is handed over."""
    import xchu_slam_amd as xa
    true, est, loops = S.circle(65)
    stages = [(45, [l for l in loops if l[1] < 45]), (55, [l for l in loops if 45 <= l[1] < 55]), (65, [l for l in loops if l[1] >= 55])]
    with xa.PoseGraph() as live, xa.PoseGraph() as only:
        have = 0
        for stage, (n, new) in enumerate(stages):
            for pg in (live, only):
                for P in est[have:n]:
                    pg.add_node(P)
                for i, j, Z, var, k in new:
                    pg.add_loop(i, j, Z, var, k)
            have = n
            live.set_solver("direct" if stage == 1 else "cg")
            info = live.optimize()
            assert live.solver_stats()["solver"] == live.solver == ("direct" if stage == 1 else "cg")
            assert (info["cg_iterations"] == 0) == (stage == 1)
            if stage == 1:
                # the CG-only graph continues from the estimate the live one reached, whichever solver reached it
                for k, P in enumerate(live.poses()):
                    only.set_estimate(k, P)
            else:
                info_only = only.optimize()
                assert info == info_only and live.poses().tobytes() == only.poses().tobytes()
                assert live.weights().tobytes() == only.weights().tobytes() and live.history() == only.history()


def test_errors():
    """An unknown solver; d over the limit (position factors on a short chain: nothing large is factorised); a residual
    rotation within 1e-6 of pi (test_gpu_pgo.test_errors' input) and a cost that leaves the finite range: the same
    status and message as under CG, and the estimate unchanged."""
    import xchu_slam_amd as xa
    from xchu_slam_amd._lib import NDT_EINVAL, NDT_EOVERFLOW, NdtError
    true, est, loops = S.circle(24, loop_every=3, max_loops=4)
    with pytest.raises(ValueError):
        xa.PoseGraph(solver="qr")
    with device_graph(xa, est, loops[:1]) as pg:
        for value in (2, -1):
            with pytest.raises(NdtError) as ei:
                pg.set_solver(value)
            assert ei.value.status == NDT_EINVAL and "unknown pose-graph solver" in str(ei.value)
        assert pg.solver == "cg"
        pg.set_solver(1)
        assert pg.solver == "direct"
        var = loops[1][3]
        half = R.exp_se3(np.array([0.0, 0.0, np.pi - 1e-7, 0.0, 0.0, 0.0]))
        pg.add_loop(2, 14, R.inv_se3(est[2]) @ est[14] @ half, var)
        for solver in ("direct", "cg"):
            pg.set_solver(solver)
            with pytest.raises(NdtError) as ei:
                pg.optimize()
            assert ei.value.status == NDT_EINVAL and "within 1e-6 of pi at between factor 1" in str(ei.value)
            assert np.array_equal(pg.poses(), est)
    far = est[:6].copy()
    far[3, :3, 3] = [1e200, 0.0, 0.0]
    with device_graph(xa, far, [(0, 5, R.inv_se3(est[0]) @ est[5], loops[0][3], 1.0)]) as pg:
        for solver in ("direct", "cg"):
            pg.set_solver(solver)
            with pytest.raises(NdtError) as ei:
                pg.optimize()
            assert ei.value.status == NDT_EOVERFLOW and "left the finite range" in str(ei.value)
            assert np.array_equal(pg.poses(), far)
    npos = LIMIT // 3 + 1
    with device_graph(xa, est[:3], [], [(k % 3, est[k % 3, :3, 3], np.array(PS.ALT_VAR), 1.0) for k in range(npos)], solver="direct") as pg:
        with pytest.raises(NdtError) as ei:
            pg.optimize()
        assert ei.value.status == NDT_EINVAL and f"d = 6 m + 3 np = {3 * npos}" in str(ei.value) and f"limit of {LIMIT}" in str(ei.value)
        assert np.array_equal(pg.poses(), est[:3])
        pg.set_solver("cg")
        assert pg.optimize()["converged"]
