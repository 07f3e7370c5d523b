"""Position factors of the pose-graph optimiser on the device (xa.PoseGraph.add_position, xa.gps_factors, the positions=
argument of xa.optimize_loops: pgo_node's gtsam::GPSFactor under useGPS) against tests/pgo_position_restate.py on the
graphs of tests/pgo_position_scene.py.

Pose tolerance, as in tests/test_gpu_pgo.py: ten times the spread of the restatement against itself on the same graphs,
measured on the CPU (dense lstsq against sparse normal equations, step_eps 1e-10 against 1e-12;
tests/test_pgo_position_restate.py repeats the measurement), the largest of each graph class:
  circles up to 65 nodes with altitude factors: the 40-node chain without loops (2.67e-14: its second step is 1e-14, so
      the stopping rule is not exercised), the 65-node circle with 7 loops (1.144e-11), its Gaussian (1.142e-11) and
      outlier (1.141e-11) variants; the two linear solves differ by 2.3e-14 at most                      1.15e-11
  the 65-node circle without loops, tight 3-D factors on every 8th node (25 iterations; solves 3.6e-14)   2.82e-11
  the 519-node hub graph with 520 altitude factors (sparse only: step_eps pair; 24 iterations)            3.27e-11
  the drifted 102-keyframe route with 34 altitude factors of variance 1e-2 (23 iterations; solves 7.1e-14) 4.08e-11
As there, the reweighted iteration converges linearly, so a run stopped at step_eps is a few step_eps from the stationary
point; that distance, not rounding, is the spread, and convergence is judged by the restatement's own Gauss-Newton step at
the device's poses, not by what the device reports.
"""
import numpy as np
import pytest

import pgo_position_restate as PR
import pgo_position_scene as PS

pytestmark = pytest.mark.gpu

STEP_EPS = 1e-10


def tol(cls):
    return 10 * PS.SPREAD[cls]


def device_graph(xa, est, loops, positions=(), **params):
    pg = xa.PoseGraph(**params)
    for P in est:
        pg.add_node(P)
    for i, j, Z, var, k in loops:
        pg.add_loop(i, j, Z, var, k)
    for node, xyz, var, k in positions:
        pg.add_position(node, xyz, var, k)
    return pg


_restated = {}


def restated(scene, solver):
    """The restatement's optimum of a scene, computed once."""
    if (scene, solver) not in _restated:
        true, est, loops, pos = scene()[:4]
        g = PR.build(est, loops, pos)
        Xr, ir = g.optimize(solver=solver, step_eps=STEP_EPS)
        assert ir["converged"]
        Xr.setflags(write=False)
        _restated[scene, solver] = (true, est, loops, pos, g, Xr)
    return _restated[scene, solver]


def position_weight_tol(g, Xr, cls):
    """|dw| of w = k^2 / (k^2 + s), s = sum r_i^2 / var_i, when the one pose of the factor moves by tol: each of the three
    residual components moves by up to tol, so ds <= 2 sqrt(s) sqrt(3) tol / sigma_min and dw = w^2 ds / k^2 (k == 0:
    w is 1 whatever the pose)."""
    r = g.position_residuals(Xr)
    s, w, _ = g._probust(r)
    _, _, var, k = g._parrays()
    k2 = np.where(k > 0, k * k, np.inf)
    return (w ** 2) * 2 * np.sqrt(3 * s) * tol(cls) / np.sqrt(var.min(1)) / k2 + 8 * np.finfo(float).eps


def between_weight_tol(g, Xr, cls):
    """tests/test_gpu_pgo.py's weight_tol."""
    _, e = g.residuals(Xr)
    s, w, _ = g._robust(e)
    lo = ~np.array(g.odom, bool)
    if not lo.any():
        return np.zeros(0)
    sig = np.sqrt(np.array(g.var)[lo].min(1))
    return (w[lo] ** 2) * 2 * np.sqrt(6 * s[lo]) * 2 * np.sqrt(6) * tol(cls) / sig + 8 * np.finfo(float).eps


def compare(scene, cls, solver="sparse"):
    """One optimise on the device and in the restatement; returns (device poses, restatement poses, graph, info, position
    weights)."""
    import xchu_slam_amd as xa
    true, est, loops, pos, g, Xr = restated(scene, solver)
    with device_graph(xa, est, loops, pos) as pg:
        info = pg.optimize()
        X, w, pw, hist = pg.poses(), pg.weights(), pg.position_weights(), pg.history()
    assert np.all(np.isfinite(X)) and np.all(X[:, 3] == [0, 0, 0, 1])
    assert info["converged"] and info["iterations"] == len(hist) >= 1
    assert info["cg_iterations"] == sum(r["cg_iterations"] for r in hist)
    assert hist[0]["cost"] == info["cost0"] and hist[-1]["max_step"] == info["max_step"] < STEP_EPS
    step = np.abs(g.gn_step_at(X, solver)).max()
    worst = np.abs(X - Xr).max()
    print(f"{scene.__name__}: iterations {info['iterations']}, restatement's step at the device's poses {step:.3e}, |X - Xr| {worst:.3e} "
          f"(tolerance {tol(cls):.3e}), cost {info['cost']!r} against {g.cost(X)!r}")
    # convergence, by the restatement's step at the device's poses
    assert step < 10 * STEP_EPS
    assert worst <= tol(cls), worst
    assert abs(info["cost"] - g.cost(X)) <= 1e-9 * max(1.0, info["cost"]) and abs(info["cost0"] - g.cost(est)) <= 1e-9 * max(1.0, info["cost0"])
    assert len(w) == len(loops) and len(pw) == len(pos)
    dpw, dw = np.abs(pw - g.position_weights(Xr)), np.abs(w - g.weights(Xr))
    print(f"{scene.__name__}: position weights off by {dpw.max():.3e} at most, between weights by {dw.max() if len(dw) else 0.0:.3e}")
    assert np.all(dpw <= position_weight_tol(g, Xr, cls))
    assert np.all(dw <= between_weight_tol(g, Xr, cls))
    return X, Xr, g, info, pw


def test_chain_with_altitude_factors():
    """A 40-node chain with no loops, the drifted z of circle(40), the true altitude on every 5th node with pgo_node's
    variances (1e9, 1e9, 250) and k = 1: the optimum moves off the input (4e-5 m: the factors are weak by design)."""
    X, Xr, g, info, pw = compare(PS.chain, "circle", "lstsq")
    est = np.array(g.init)
    assert len(pw) == 8 and np.all(pw > 0.99) and np.all(pw <= 1.0)
    assert 1e-6 < np.abs(X - est).max() < 1e-3 and info["cost"] < info["cost0"]


def test_circle_with_loops_and_altitude_factors():
    """circle(65) with its 7 loops; altitude factors on node 0 (which has the prior), on 63 and 64 (the last lane of one
    wave, the first of the next; 64 is the last node), and two on node 20."""
    true, est, loops, pos = PS.circle()
    nodes = [p[0] for p in pos]
    assert len(loops) == 7 and {0, 63, 64} <= set(nodes) and nodes.count(20) == 2
    X, Xr, g, info, pw = compare(PS.circle, "circle", "lstsq")
    assert pw[1] != pw[4] and info["cost"] < info["cost0"]


def test_hub_graph_with_a_factor_on_every_node():
    """519 nodes (runs of two nodes per thread in the scans) with an altitude factor each and a second one on the hub
    node: 520 factors for 512 threads, and the hub's gather walks 70 edges and then 2 position factors."""
    true, est, loops, pos = PS.hub()
    assert len(pos) == PS.THREADS + 8 and sum(1 for p in pos if p[0] == 10) == 2 and sum(1 for l in loops if 10 in l[:2]) >= 70
    compare(PS.hub, "hub")


def test_tight_three_axis_factors():
    """True positions with variance 1e-2 on all three axes on every 8th node of circle(65), no loops: the optimum is
    more than 5 cm off the drifted odometry in each of x, y and z, so a wrong sign or transpose in K = [-hat(t) I]
    (|t| = 20 m) cannot pass the pose comparison."""
    X, Xr, g, info, pw = compare(PS.tight, "tight", "lstsq")
    est = np.array(g.init)
    assert np.all(np.abs(X - est)[:, :3, 3].max(0) > 0.05) and info["cost"] < info["cost0"]


def test_gaussian_factor():
    """robust_k = 0: the weight is exactly 1."""
    X, Xr, g, info, pw = compare(PS.gaussian, "circle", "lstsq")
    assert pw[2] == 1.0 and np.all(np.delete(pw, [0, 2]) < 1.0)      # (node 0 sits on its measurement)


def test_gross_outlier_is_down_weighted():
    """One altitude 500 m off: its weight equals the restatement's (compare) and is below every other position weight."""
    X, Xr, g, info, pw = compare(PS.outlier, "circle", "lstsq")
    pr = g.position_weights(Xr)
    assert pw[2] < 0.01 and np.all(pw[2] < np.delete(pw, 2)) and np.all(pr[2] < np.delete(pr, 2))


def test_warm_start():
    """circle(65): optimise with the loops and the first three altitude factors, add the other four, optimise again: the
    optimum of one optimise of the whole graph, in fewer iterations (the restatement takes 14, then 8 against 14)."""
    import xchu_slam_amd as xa
    true, est, loops, pos = PS.circle()
    with device_graph(xa, est, loops, pos) as whole:
        info_whole = whole.optimize()
        X_whole = whole.poses()
    with device_graph(xa, est, loops, pos[:3]) as pg:
        info1 = pg.optimize()
        assert info1["converged"] and len(pg.position_weights()) == 3
        for node, xyz, var, k in pos[3:]:
            pg.add_position(node, xyz, var, k)
        assert len(pg.position_weights()) == 3           # of the last optimise
        info2 = pg.optimize()
        X2, pw2 = pg.poses(), pg.position_weights()
        assert len(pw2) == len(pos) and len(pg.weights()) == len(loops)
    print(f"warm start: {info1['iterations']} + {info2['iterations']} iterations, whole graph {info_whole['iterations']}, "
          f"|X2 - X_whole| {np.abs(X2 - X_whole).max():.3e}")
    assert info_whole["converged"] and info2["converged"] and info2["iterations"] < info_whole["iterations"]
    assert np.abs(X2 - X_whole).max() <= tol("circle")
    g, Xr = restated(PS.circle, "lstsq")[4:]
    assert np.abs(g.gn_step_at(X2, "lstsq")).max() < 10 * STEP_EPS and np.abs(X2 - Xr).max() <= tol("circle")
    assert np.all(np.abs(pw2 - g.position_weights(Xr)) <= position_weight_tol(g, Xr, "circle"))


def test_determinism():
    """Two runs on the same input give bitwise equal poses, both weight arrays and records."""
    import xchu_slam_amd as xa
    true, est, loops, pos = PS.hub()
    out = []
    for _ in range(2):
        with device_graph(xa, est, loops, pos) as pg:
            info = pg.optimize()
            out.append((pg.poses(), pg.weights(), pg.position_weights(), info, pg.history()))
    assert all(out[0][k].tobytes() == out[1][k].tobytes() for k in range(3)) and len(out[0][2]) == len(pos)
    assert out[0][3] == out[1][3] and out[0][4] == out[1][4]


def test_errors():
    """A node out of range, a non-finite coordinate, a variance that is not finite and positive and a negative robust_k
    each give NDT_EINVAL and a message; the graph and the estimate stay as they were."""
    import xchu_slam_amd as xa
    from xchu_slam_amd._lib import NDT_EINVAL, NdtError
    true, est, loops, pos = PS.circle()
    with device_graph(xa, est, loops, pos[:2]) as pg:
        info = pg.optimize()
        X, pw = pg.poses(), pg.position_weights()
        xyz, var = pos[2][1], pos[2][2]

        def bad(call, text):
            with pytest.raises(NdtError) as ei:
                call()
            assert ei.value.status == NDT_EINVAL and text in str(ei.value), str(ei.value)

        bad(lambda: pg.add_position(65, xyz, var), "position factor: node index out of range")
        bad(lambda: pg.add_position(-1, xyz, var), "position factor: node index out of range")
        bad(lambda: pg.add_position(3, [1.0, np.nan, 0.0], var), "position factor: position is not finite")
        bad(lambda: pg.add_position(3, [np.inf, 0.0, 0.0], var), "position factor: position is not finite")
        bad(lambda: pg.add_position(3, xyz, [1.0, 0.0, 1.0]), "position factor: variances")
        bad(lambda: pg.add_position(3, xyz, [1.0, -1.0, 1.0]), "position factor: variances")
        bad(lambda: pg.add_position(3, xyz, [1.0, np.inf, 1.0]), "position factor: variances")
        bad(lambda: pg.add_position(3, xyz, [np.nan, 1.0, 1.0]), "position factor: variances")
        bad(lambda: pg.add_position(3, xyz, var, robust_k=-1.0), "position factor: robust k")
        with pytest.raises(ValueError):
            pg.add_position(3, [1.0, 2.0], var)
        assert len(pg) == 65 and np.array_equal(pg.poses(), X) and np.array_equal(pg.position_weights(), pw)
        # none of them was stored: a second optimise is a warm start of the same graph
        again = pg.optimize()
        assert again["converged"] and again["iterations"] <= 2 and len(pg.position_weights()) == 2
        assert np.abs(pg.poses() - X).max() <= tol("circle")
    assert info["converged"]


def test_optimize_loops_with_gps_factors_on_the_drifted_route():
    """xa.optimize_loops(est, accepted, positions=xa.gps_factors(...)) on the drifted Scan Context route (a fix 0.03 s
    after every third keyframe, altitude variance 1e-2: tests/pgo_position_scene.py says why): the restatement's poses,
    and a z-RMS against the truth below that of the loops alone."""
    import xchu_slam_amd as xa
    true, est, loops, pos, accepted = PS.route()
    kt = 10.0 + 0.5 * np.arange(len(est))
    sel = np.arange(0, len(est), 3)
    factors = xa.gps_factors(kt, est, kt[sel] + 0.03, 120.0 + true[sel, 2, 3], altitude_var=1e-2)
    assert len(factors) == len(pos) == 34 and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(factors, pos))
    g = PR.build(est, loops, pos)
    Xr, ir = g.optimize(solver="sparse", step_eps=STEP_EPS)
    X0, i0 = PR.build(est, loops).optimize(solver="sparse", step_eps=STEP_EPS)
    zrms = lambda A: np.sqrt(((A - true)[:, 2, 3] ** 2).mean())
    assert ir["converged"] and i0["converged"] and zrms(Xr) < 0.5 * zrms(X0) < zrms(est)      # the input condition (also a CPU test)
    poses6d, info = xa.optimize_loops(est, accepted, positions=factors)
    _, info0 = xa.optimize_loops(est, accepted)
    worst = np.abs(info["poses"] - Xr).max()
    print(f"route: iterations {info['iterations']}, |X - Xr| {worst:.3e} (tolerance {tol('route'):.3e}), z-RMS {zrms(info['poses']):.4f} m, "
          f"loops alone {zrms(info0['poses']):.4f} m")
    assert info["converged"] and poses6d.shape == (len(est), 6)
    assert worst <= tol("route")
    assert np.abs(g.gn_step_at(info["poses"], "sparse")).max() < 10 * STEP_EPS
    assert abs(info["cost"] - g.cost(info["poses"])) <= 1e-9 * max(1.0, info["cost"])
    assert len(info["position_weights"]) == 34 and len(info["weights"]) == len(accepted)
    assert np.all(np.abs(info["position_weights"] - g.position_weights(Xr)) <= position_weight_tol(g, Xr, "route"))
    assert zrms(info["poses"]) < zrms(info0["poses"]) and zrms(info["poses"]) < 0.5 * zrms(X0)
    assert len(info0["position_weights"]) == 0
