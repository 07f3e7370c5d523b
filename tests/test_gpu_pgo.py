"""The pose-graph optimiser on the device (xa.PoseGraph, xa.optimize_loops) against tests/pgo_restate.py on synthetic
two-lap circles with drifted odometry and loops every few keyframes (tests/pgo_scene.py).

Pose tolerance: ten times the spread of the restatement against itself on the same graphs, measured on the CPU
(dense lstsq against sparse normal equations, step_eps 1e-10 against 1e-12), the largest of each graph class:
  circles up to 65 nodes (with the reversed, Gaussian and outlier variants)  1.14e-11  (the step_eps pair; the two
      linear solves differ by 4e-14)
  the 519-node hub graph                                                      3.29e-11  (sparse only: step_eps pair)
  the drifted 102-keyframe route                                              1.52e-10  (79 iterations at rate 0.8)
The reweighted iteration converges linearly, so a run stopped at step_eps is a few step_eps from the stationary point;
that distance, not rounding, is the spread.  Convergence is judged by the restatement's own Gauss-Newton step at the
device's poses, not by what the device reports.
"""
import numpy as np
import pytest

import pgo_restate as R
import pgo_scene as S
import sc_scene

pytestmark = pytest.mark.gpu

STEP_EPS = 1e-10
SPREAD = {"circle": 1.14e-11, "hub": 3.29e-11, "route": 1.52e-10}
THREADS = 512     # ndt::kPgoBlock


def tol(cls):
    return 10 * SPREAD[cls]


def device_graph(xa, est, loops, **params):
    pg = xa.PoseGraph(**params)
    for P in est:
        pg.add_node(P)
    for i, j, Z, var, k in loops:
        pg.add_loop(i, j, Z, var, k)
    return pg


def compare(est, loops, cls, solver="sparse"):
    """One optimise on the device and in the restatement; returns (device poses, restatement poses, graph, info, w)."""
    import xchu_slam_amd as xa
    g = R.build(est, loops)
    Xr, ir = g.optimize(solver=solver, step_eps=STEP_EPS)
    assert ir["converged"]
    with device_graph(xa, est, loops) as pg:
        info = pg.optimize()
        X, w, hist = pg.poses(), pg.weights(), pg.history()
    assert np.all(np.isfinite(X)) and np.all(X[:, 3] == [0, 0, 0, 1])
    assert info["converged"] and info["iterations"] == len(hist) >= 1
    assert info["cg_iterations"] == sum(r["cg_iterations"] for r in hist)
    assert hist[0]["cost"] == info["cost0"] and hist[-1]["max_step"] == info["max_step"] < STEP_EPS
    # convergence, by the restatement's step at the device's poses
    assert np.abs(g.gn_step_at(X, solver)).max() < 10 * STEP_EPS
    assert np.abs(X - Xr).max() <= tol(cls), np.abs(X - Xr).max()
    assert abs(info["cost"] - g.cost(X)) <= 1e-9 * max(1.0, info["cost"]) and abs(info["cost0"] - g.cost(est)) <= 1e-9 * max(1.0, info["cost0"])
    assert len(w) == len(loops)
    return X, Xr, g, info, w


def weight_tol(g, Xr, cls):
    """|dw| of w = k^2 / (k^2 + s) when every residual component moves by up to sqrt(6) tol (a pose moves by tol):
    ds <= 2 sqrt(s) sqrt(6) tol' / sigma with tol' = 2 sqrt(6) tol for the two poses of the edge, dw = w^2 ds / k^2."""
    _, e = g.residuals(Xr)
    s, w, _ = g._robust(e)
    lo = ~np.array(g.odom)
    sig = np.sqrt(np.array(g.var)[lo].min(1))
    return (w[lo] ** 2) * 2 * np.sqrt(6 * s[lo]) * 2 * np.sqrt(6) * tol(cls) / sig + 8 * np.finfo(float).eps


def test_single_node():
    """n = 1: the prior alone; the pose comes back bit for bit."""
    import xchu_slam_amd as xa
    _, est, _ = S.circle(24)
    with device_graph(xa, est[:1], []) as pg:
        info = pg.optimize()
        assert info["converged"] and info["cost0"] == 0.0 == info["cost"] and info["max_step"] == 0.0
        assert np.array_equal(pg.poses(), est[:1]) and len(pg) == 1 and len(pg.weights()) == 0
        assert np.abs(pg.poses6d() - R.rpy(est[:1])).max() == 0.0


def test_two_nodes_and_no_loops():
    """n = 2, and a 40-node chain without loops: the input is the optimum (within 1e-12, as the restatement's)."""
    _, est, _ = S.circle(40)
    for n in (2, 40):
        X, Xr, _, info, _ = compare(est[:n], [], "circle", "lstsq")
        assert np.abs(X - est[:n]).max() < 1e-12 and info["iterations"] == 1


@pytest.mark.parametrize("n,kw", [(24, dict(loop_every=3, max_loops=4)), (65, {})])
def test_circle(n, kw):
    """24 nodes with 4 loops, 65 nodes with 7 (one node more than a wave)."""
    true, est, loops = S.circle(n, **kw)
    assert len(loops) == (4 if n == 24 else 7)
    X, Xr, g, info, w = compare(est, loops, "circle", "lstsq")
    assert np.all(np.abs(w - g.weights(Xr)) <= weight_tol(g, Xr, "circle"))
    assert info["cost"] < info["cost0"]


def test_hub_graph():
    """More nodes than the workgroup has threads plus an odd remainder, more than 64 loop edges, and a hub node that is
    an endpoint of 70 of them (its gather walks a 70-entry edge list)."""
    true, est, loops = S.hub(THREADS + 7)
    assert len(loops) > 64 + 7 and sum(1 for l in loops if 10 in l[:2]) >= 70
    X, Xr, g, info, w = compare(est, loops, "hub")
    assert np.all(np.abs(w - g.weights(Xr)) <= weight_tol(g, Xr, "hub"))


def test_reversed_loops():
    """Loops given as (j, i) with j > i and the inverted measurement.  (Not the forward graph's problem: the residual
    becomes -Ad(Z) e, whose whitened norm differs, so the comparison is with the restatement of the reversed graph.)"""
    true, est, loops = S.circle(65)
    rev = [(j, i, R.inv_se3(Z), var, k) for i, j, Z, var, k in loops]
    assert all(i > j for i, j, *_ in rev)
    X, Xr, g, _, w = compare(est, rev, "circle", "lstsq")
    assert np.all(np.abs(w - g.weights(Xr)) <= weight_tol(g, Xr, "circle"))


def test_gaussian_loop():
    """One loop with k = 0: weight exactly 1."""
    true, est, loops = S.circle(65)
    loops[2] = loops[2][:4] + (0.0,)
    X, Xr, g, info, w = compare(est, loops, "circle", "lstsq")
    assert w[2] == 1.0 and np.all(w[[0, 1, 3, 4, 5, 6]] < 1.0)
    assert np.all(np.abs(w - g.weights(Xr)) <= weight_tol(g, Xr, "circle"))


def test_gross_outlier_is_down_weighted():
    """One loop whose measurement is 10 m off: its final weight equals the restatement's and is below every inlier's."""
    true, est, loops = S.circle(65)
    Z = loops[3][2].copy()
    Z[:3, 3] += [10.0, 0.0, 0.0]
    loops[3] = (loops[3][0], loops[3][1], Z) + loops[3][3:]
    X, Xr, g, info, w = compare(est, loops, "circle", "lstsq")
    wr = g.weights(Xr)
    assert np.all(np.abs(w - wr) <= weight_tol(g, Xr, "circle"))
    assert w[3] < 0.01 and np.all(w[3] < np.delete(w, 3)) and np.all(wr[3] < np.delete(wr, 3))


def test_warm_start():
    """Ten nodes and two loops added after an optimise, then a second optimise: the optimum of one optimise of the
    whole graph, in fewer iterations."""
    import xchu_slam_amd as xa
    true, est, loops = S.circle(65)
    first = [l for l in loops if l[1] < 55]
    rest = [l for l in loops if l[1] >= 55]
    assert len(rest) == 2
    with device_graph(xa, est, loops) as whole:
        info_whole = whole.optimize()
        X_whole = whole.poses()
    with device_graph(xa, est[:55], first) as pg:
        info1 = pg.optimize()
        assert info1["converged"]
        for P in est[55:]:
            pg.add_node(P)
        for i, j, Z, var, k in rest:
            pg.add_loop(i, j, Z, var, k)
        assert np.array_equal(pg.poses()[55:], est[55:])     # a new node's estimate is its pose as given
        info2 = pg.optimize()
        X2 = pg.poses()
        assert len(pg.weights()) == len(loops)
    assert info2["converged"] and info2["iterations"] < info_whole["iterations"]
    assert np.abs(X2 - X_whole).max() <= tol("circle")
    g = R.build(est, loops)
    assert np.abs(g.gn_step_at(X2, "lstsq")).max() < 10 * STEP_EPS


def test_determinism():
    """Two runs on the same input give bitwise equal poses, weights and records."""
    import xchu_slam_amd as xa
    true, est, loops = S.hub(THREADS + 7)
    out = []
    for _ in range(2):
        with device_graph(xa, est, loops) as pg:
            info = pg.optimize()
            out.append((pg.poses(), pg.weights(), info, pg.history()))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3]


def test_errors():
    """i == j, an index out of range, a non-finite or non-rigid pose, bad variances, and a residual rotation within 1e-6
    of pi each give an error status and a message; the estimate stays finite and unchanged."""
    import xchu_slam_amd as xa
    from xchu_slam_amd._lib import NDT_EINVAL, NdtError
    true, est, loops = S.circle(24, loop_every=3, max_loops=4)
    with device_graph(xa, est, loops[:1]) as pg:
        Z, var = loops[1][2], loops[1][3]

        def bad(call, text):
            with pytest.raises(NdtError) as ei:
                call()
            assert ei.value.status == NDT_EINVAL and text in str(ei.value), str(ei.value)

        bad(lambda: pg.add_loop(3, 3, Z, var), "i == j")
        bad(lambda: pg.add_loop(3, 24, Z, var), "out of range")
        bad(lambda: pg.add_loop(-1, 3, Z, var), "out of range")
        nan = est[5].copy()
        nan[1, 3] = np.nan
        bad(lambda: pg.add_node(nan), "finite rigid")
        bad(lambda: pg.add_loop(3, 9, nan, var), "finite rigid")
        bad(lambda: pg.add_node(2.0 * est[5]), "finite rigid")
        bad(lambda: pg.add_loop(3, 9, Z, np.array([1, 1, 0, 1, 1, 1.0])), "variances")
        bad(lambda: pg.add_loop(3, 9, Z, var, robust_k=-1.0), "robust k")
        assert len(pg) == 24 and len(pg.weights()) == 0
        # a measurement half a turn (less 1e-7 rad) away from what the poses say
        half = R.exp_se3(np.array([0.0, 0.0, np.pi - 1e-7, 0.0, 0.0, 0.0]))
        pg.add_loop(2, 14, R.inv_se3(est[2]) @ est[14] @ half, var)
        bad(pg.optimize, "within 1e-6 of pi at between factor 1")
        assert np.array_equal(pg.poses(), est)
    with pytest.raises(TypeError):
        xa.PoseGraph(no_such_parameter=1)
    with pytest.raises(NdtError):
        xa.PoseGraph(max_iter=0)


def test_optimize_loops_on_the_drifted_route():
    """xa.optimize_loops with records as close_loops returns them (built from the truth: no ICP run) on the drifted Scan
    Context route: the restatement's poses; the literal measurement is the reference's BetweenFactor."""
    import xchu_slam_amd as xa
    true, est, accepted = S.drifted_route(sc_scene.route_poses())
    loops = [(i, j, xa.loop_measurement(est, i, j, T), np.full(6, s), 1.0) for i, j, T, s in accepted]
    g = R.build(est, loops)
    Xr, ir = g.optimize(solver="sparse", step_eps=STEP_EPS)
    rms = lambda A: np.sqrt(((A - true)[:, :3, 3] ** 2).sum(1).mean())
    assert ir["converged"] and rms(Xr) < 0.5 * rms(est)           # the input condition (also a CPU test)
    poses6d, info = xa.optimize_loops(est, accepted)
    assert info["converged"] and poses6d.shape == (len(est), 6)
    assert np.abs(info["poses"] - Xr).max() <= tol("route")
    assert np.abs(g.gn_step_at(info["poses"], "sparse")).max() < 10 * STEP_EPS
    d = poses6d - R.rpy(Xr)
    d[:, 3:] = (d[:, 3:] + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() <= 2 * tol("route")                    # an angle is an arctangent of two entries
    assert rms(info["poses"]) < 0.5 * rms(est)
    # poses given as (x, y, z, roll, pitch, yaw) build the same graph up to the rounding of Pose6D2Matrix
    p6, _ = xa.optimize_loops(R.rpy(est), accepted)
    assert np.abs(p6[:, :3] - poses6d[:, :3]).max() < 1e-9
    # the literal form builds the reference's factor, Z = T_icp^-1 whatever the poses are: the cost at the input says so
    # (its reweighted iteration needs more than 200 steps here, so only the first step is taken)
    lit = [(i, j, xa.loop_measurement(est, i, j, T, True), np.full(6, s), 1.0) for i, j, T, s in accepted]
    gl = R.build(est, lit)
    _, info_l = xa.optimize_loops(est, accepted, literal_measurement=True, max_iter=1)
    assert info_l["iterations"] == 1 and not info_l["converged"]
    assert abs(info_l["cost0"] - gl.cost(est)) <= 1e-9 * gl.cost(est) and abs(gl.cost(est) - g.cost(est)) > 1.0
    assert abs(info_l["cost"] - gl.cost(info_l["poses"])) <= 1e-9 * gl.cost(est)


def test_shares_a_registration_context():
    """A PoseGraph on an existing registration's context (its device and stream) leaves that registration usable, and is
    closed before it."""
    import xchu_slam_amd as xa
    from helpers import small_pair
    pair = small_pair(seed=3, n_source=1000)
    true, est, loops = S.circle(24, loop_every=3, max_loops=4)
    with xa.NormalDistributionsTransform() as ndt:
        ndt.setInputTarget(pair.target)
        ndt.setInputSource(pair.source)
        ndt.align(pair.guess)
        T = ndt.getFinalTransformation()
        pg = device_graph(xa, est, loops, registration=ndt)
        assert pg.registration is ndt and pg.ctx is ndt.ctx
        assert pg.optimize()["converged"]
        X = pg.poses()
        pg.close()
        ndt.align(pair.guess)
        assert np.array_equal(np.asarray(ndt.getFinalTransformation()).view(np.uint32), np.asarray(T).view(np.uint32))
    with device_graph(xa, est, loops) as own:
        own.optimize()
        assert own.poses().tobytes() == X.tobytes()
