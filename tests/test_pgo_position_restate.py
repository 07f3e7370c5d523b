"""Pins tests/pgo_position_restate.py (tests/pgo_restate.py with pgo_node's GPS position factors, DESIGN.md §2 "Pose
graph"), xa.gps_factors, and measures the restatement's spread on the graphs of tests/test_gpu_pgo_position.py.  No GPU."""
import numpy as np
import pytest

import pgo_position_restate as PR
import pgo_position_scene as PS
import pgo_restate as R
import pgo_scene as S
import sc_scene

EPS = np.finfo(np.float64).eps


def test_without_position_factors_it_is_the_parent_class_bit_for_bit():
    true, est, loops = S.circle(24, loop_every=3, max_loops=4)
    a, b = R.build(est, loops), PR.build(est, loops)
    same = lambda x, y: np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).shape == np.asarray(y).shape
    assert all(same(x, y) for x, y in zip(a.residuals(est), b.residuals(est)))
    assert same(a.weights(est), b.weights(est)) and a.cost(est) == b.cost(est)
    assert all(same(x, y) for x, y in zip(a.linearize(est), b.linearize(est)))
    assert b.position_residuals(est).shape == (0, 3) and b.position_weights(est).shape == (0,)
    for solver in ("lstsq", "sparse"):
        assert same(a.gn_step_at(est, solver), b.gn_step_at(est, solver))
        (Xa, ia), (Xb, ib) = a.optimize(solver=solver), b.optimize(solver=solver)
        assert same(Xa, Xb) and ib.pop("position_weights").shape == (0,) and ia == ib


def test_jacobian_against_central_differences():
    """dr/dd = [0 R] for r = t(X Exp(d)) - z, and the form the kernel uses, dr/du = [-hat(t) I] for the world-frame
    u = Ad(X) d (X Exp(d) = Exp(u) X), at poses 20 m from the origin with rotations of 0.7 to 2.5 rad: hat(t) is then
    the largest entry.  Central differences with h = 1e-5: r is t + R V(w) v, smooth with third derivatives O(|t|) = 20
    in u, so truncation h^2/6 * 20 = 3e-10 and round-off eps |t| / h = 4e-10 stay below 1e-8."""
    rng = np.random.default_rng(5)
    h = 1e-5
    for angle in (0.7, 1.6, 2.5):
        w = rng.normal(size=3)
        t = rng.normal(size=3)
        X = R.exp_se3(np.concatenate([w / np.linalg.norm(w) * angle, np.zeros(3)]))
        X[:3, 3] = t / np.linalg.norm(t) * 20.0
        g = PR.build([X], [], [(0, X[:3, 3] + [0.3, -0.2, 0.1], np.array([0.5, 2.0, 250.0]), 1.0)])
        J = g.position_jacobian(X[None])[0]
        assert np.array_equal(J[:, :3], np.zeros((3, 3))) and np.array_equal(J[:, 3:], X[:3, :3])
        num = np.zeros((3, 6))
        world = np.zeros((3, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            num[:, k] = (g.position_residuals((X @ R.exp_se3(d))[None])[0] - g.position_residuals((X @ R.exp_se3(-d))[None])[0]) / (2 * h)
            world[:, k] = (g.position_residuals((R.exp_se3(d) @ X)[None])[0] - g.position_residuals((R.exp_se3(-d) @ X)[None])[0]) / (2 * h)
        assert np.abs(num - J).max() < 1e-8
        K = np.concatenate([-R.hat(X[:3, 3]), np.eye(3)], 1)
        assert np.abs(world - K).max() < 1e-8 and np.abs(K).max() > 10.0
        assert np.abs(J @ R.adjoint(R.inv_se3(X)) - K).max() < 64 * EPS * 20.0
        # the whitened, weighted rows: sqrt(w / var) times the above
        r = g.position_residuals(X[None])[0]
        s = np.sum(r * r / [0.5, 2.0, 250.0])
        rows, Jw, node = g.linearize_positions(X[None])
        assert abs(g.position_weights(X[None])[0] - 1 / (1 + s)) < 4 * EPS and node.tolist() == [0]
        assert np.abs(rows[0] - r * np.sqrt(1 / (1 + s) / np.array([0.5, 2.0, 250.0]))).max() < 4 * EPS
        assert np.abs(Jw[0] - J * np.sqrt(1 / (1 + s) / np.array([0.5, 2.0, 250.0]))[:, None]).max() < 4 * EPS
        assert abs(g.cost(X[None]) - 0.5 * np.log1p(s)) < 16 * EPS


def test_robust_weight_and_cost_of_a_position_factor():
    """Cauchy as for a between factor; k == 0 is Gaussian with weight exactly 1."""
    X = np.eye(4)[None].copy()
    X[0, :3, 3] = [1.0, 2.0, 3.0]
    s = 0.5 ** 2 / 0.1 + 1.0 ** 2 / 0.2
    for k, w, c in ((1.0, 1 / (1 + s), 0.5 * np.log1p(s)), (2.0, 4 / (4 + s), 2 * np.log1p(s / 4)), (0.0, 1.0, 0.5 * s)):
        g = PR.build(X, [], [(0, [0.5, 3.0, 3.0], [0.1, 0.2, 0.3], k)])
        assert abs(g.position_weights(X)[0] - w) < 4 * EPS and abs(g.cost(X) - c) < 16 * EPS
        assert k or g.position_weights(X)[0] == 1.0


def test_known_answer_one_node_between_prior_and_position():
    """A Gaussian position factor on a one-node graph: the prior (variance 1e-12) and the factor (variance v) are
    averaged by their information, t = z / (1 + v / 1e-12) off the prior's mean along each axis."""
    X = np.eye(4)[None].copy()
    g = PR.build(X, [], [(0, [1.0, -2.0, 0.5], [1e-10, 1e-10, 1e-10], 0.0)])
    for solver in ("lstsq", "sparse"):
        Xo, info = g.optimize(solver=solver)
        assert info["converged"] and np.abs(Xo[0, :3, 3] - np.array([1.0, -2.0, 0.5]) / 101.0).max() < 1e-12
        assert np.abs(Xo[0, :3, :3] - np.eye(3)).max() < 1e-12


# ------------------------------------------------------------------------------------------------ xa.gps_factors
def test_gps_factors_association():
    import xchu_slam_amd as xa
    true, est, _ = S.circle(24)
    kt = 100.0 + np.arange(24.0)
    # no fixes: no factors
    assert xa.gps_factors(kt, est, [], []) == []
    # keyframe 3: a fix exactly eps away is rejected (0.125 and the times are exact in binary); keyframe 5: fixes at equal
    # distance before and after, the earlier one is taken (given in either order); keyframe 8: strictly within eps;
    # keyframe 10: nearest fix is beyond eps although an earlier keyframe's fix matched
    gt = [103.125, 105.0625, 104.9375, 108.0625, 110.5]
    alt = [500.0, 52.0, 51.0, 57.5, 60.0]
    out = xa.gps_factors(kt, est, gt, alt, eps=0.125)
    assert [o[0] for o in out] == [5, 8]
    # the offset is the altitude of the first keyframe that has GPS (the earlier of its two fixes: 51)
    assert out[0][1].tolist() == [est[5, 0, 3], est[5, 1, 3], 0.0] and out[1][1].tolist() == [est[8, 0, 3], est[8, 1, 3], 6.5]
    assert all(o[2].tolist() == [1e9, 1e9, 250.0] for o in out)
    swapped = xa.gps_factors(kt, est, [gt[i] for i in (0, 2, 1, 3, 4)], [alt[i] for i in (0, 2, 1, 3, 4)], eps=0.125)
    assert [(o[0], o[1].tolist()) for o in swapped] == [(o[0], o[1].tolist()) for o in out]
    # just inside eps on the other side; poses given as (x, y, z, roll, pitch, yaw); the variances are the arguments
    one = xa.gps_factors(kt, R.rpy(est), [102.875], [7.0], eps=0.125, altitude_var=4.0, xy_var=1e6)
    assert len(one) == 0
    one = xa.gps_factors(kt, R.rpy(est), [102.9375], [7.0], eps=0.125, altitude_var=4.0, xy_var=1e6)
    assert [o[0] for o in one] == [3] and one[0][1].tolist() == [est[3, 0, 3], est[3, 1, 3], 0.0] and one[0][2].tolist() == [1e6, 1e6, 4.0]
    with pytest.raises(ValueError):
        xa.gps_factors(kt[:5], est, gt, alt)


# ------------------------------------------------------------------------------------------------ the spread
@pytest.fixture(scope="module")
def route():
    return PS.route()


def measure(est, loops, pos, dense):
    """The restatement against itself: (spread, step-eps pair, solver pair, poses at 1e-10, graph)."""
    g = PR.build(est, loops, pos)
    Xs, i1 = g.optimize(solver="sparse", step_eps=1e-10)
    Xt, i2 = g.optimize(solver="sparse", step_eps=1e-12)
    assert i1["converged"] and i2["converged"]
    # the convergence check the GPU tests apply to the device, applied to the restatement's own result first
    assert np.abs(g.gn_step_at(Xs, "sparse")).max() < 10 * 1e-10
    eps_pair, solver_pair = np.abs(Xs - Xt).max(), 0.0
    if dense:
        Xd, i3 = g.optimize(solver="lstsq", step_eps=1e-10)
        assert i3["converged"]
        solver_pair = np.abs(Xs - Xd).max()
    return max(eps_pair, solver_pair), eps_pair, solver_pair, Xs, g


@pytest.mark.parametrize("cls", ["circle", "tight", "hub", "route"])
def test_spread_of_the_restatement(cls, route):
    """PS.SPREAD, the figure ten times which is the GPU tests' pose tolerance, is what the restatement differs from itself
    by on that class's graphs (dense lstsq against sparse normal equations, step_eps 1e-10 against 1e-12; the hub graph
    sparse only): not below the measurement, and not more than 1.5 times above it."""
    worst = 0.0
    for scene in PS.CLASSES[cls]:
        true, est, loops, pos = route[:4] if cls == "route" else scene()
        spread, eps_pair, solver_pair, _, _ = measure(est, loops, pos, dense=cls != "hub")
        print(f"{cls} {scene.__name__}: step-eps pair {eps_pair:.3e}, solver pair {solver_pair:.3e}")
        worst = max(worst, spread)
    assert worst <= PS.SPREAD[cls] <= 1.5 * worst, (cls, worst)


def test_tight_factors_pull_the_optimum_off_the_odometry():
    """The input condition of the tight GPU case: the optimum is more than 5 cm from the drifted input in each of x, y, z
    (0.18 m at most: the Cauchy kernel holds factors a metre off at weights near 0.01) and closer to the truth."""
    true, est, loops, pos = PS.tight()
    X, info = PR.build(est, loops, pos).optimize(solver="sparse")
    assert info["converged"] and np.all(np.abs(X - est)[:, :3, 3].max(0) > 0.05)
    rms = lambda A: np.sqrt(((A - true)[:, :3, 3] ** 2).sum(1).mean())
    assert rms(X) < rms(est) - 0.1, (rms(X), rms(est))


def test_drifted_route_with_altitudes_is_a_fair_input(route):
    """The input condition of the optimize_loops GPU test: with the altitude factors the restatement's optimum has a
    lower z-RMS against the truth than with the loops alone."""
    true, est, loops, pos, _ = route
    X0, i0 = PR.build(est, loops).optimize(solver="sparse")
    X, info = PR.build(est, loops, pos).optimize(solver="sparse")
    zrms = lambda A: np.sqrt(((A - true)[:, 2, 3] ** 2).mean())
    assert i0["converged"] and info["converged"] and len(pos) == 34
    assert zrms(X) < 0.5 * zrms(X0) < zrms(est), (zrms(X), zrms(X0), zrms(est))
