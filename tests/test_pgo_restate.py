"""Pins tests/pgo_restate.py, the numpy / scipy restatement of the pose-graph optimiser (the reference holds no GTSAM
source: DESIGN.md §2 "Pose graph"), and xa.loop_measurement.  No GPU."""
import numpy as np
import pytest

import pgo_restate as R
import pgo_scene as S
import sc_scene

EPS = np.finfo(np.float64).eps


def tangent(rng, angle, n=1):
    xi = rng.normal(size=(n, 6))
    w = xi[:, :3]
    xi[:, :3] = w / np.linalg.norm(w, axis=1, keepdims=True) * angle
    return xi


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-4, 0.19, 0.21, 1.0, 3.0])
def test_exp_log_round_trip(angle):
    """Log(Exp(xi)) == xi on both sides of the series threshold, at |w| == 0 exactly and at 1e-9; the bound is a few ulp
    of the tangent's size (the translation part carries |v| ~ 2)."""
    xi = tangent(np.random.default_rng(1), angle, 8)
    T = R.exp_se3(xi)
    assert np.all(np.isfinite(T))
    assert np.abs(T[:, :3, :3] @ np.swapaxes(T[:, :3, :3], 1, 2) - np.eye(3)).max() < 16 * EPS
    assert np.abs(R.log_se3(T) - xi).max() < 64 * EPS * max(1.0, np.abs(xi).max())
    assert np.abs(R.exp_se3(R.log_se3(T)) - T).max() < 64 * EPS * max(1.0, np.abs(T).max())


def test_log_rejects_rotations_at_pi():
    xi = np.array([0.0, 0.0, np.pi - 1e-7, 1.0, 2.0, 3.0])
    with pytest.raises(R.RotationNearPi):
        R.log_se3(R.exp_se3(xi))
    ok = np.array([0.0, 0.0, np.pi - 1e-5, 1.0, 2.0, 3.0])
    assert np.abs(R.log_se3(R.exp_se3(ok)) - ok).max() < 1e-9   # eps / sin(theta) in the axis


def central(f, h):
    """Central differences of f: R^6 -> R^6 at 0."""
    J = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        J[:, k] = (f(d) - f(-d)) / (2 * h)
    return J


@pytest.mark.parametrize("angle", [0.0, 1e-9, 0.1, 0.19, 0.21, 1.5, 3.0])
def test_jacobians_against_central_differences(angle):
    """de/ddj = Jr^-1(e) and de/ddi = -Jr^-1(e) Ad(Xj^-1 Xi) for e = Log(Z^-1 Xi^-1 Xj) under X <- X Exp(d).  Central
    differences with h = 1e-5: truncation h^2/6 |e'''| (third derivatives of Log are O(1 + |v|) here: |v| ~ 2) plus
    round-off eps |e| / h, together below 1e-8."""
    rng = np.random.default_rng(2)
    h = 1e-5
    Xi, Xj = R.exp_se3(tangent(rng, 0.7)[0]), R.exp_se3(tangent(rng, 1.1)[0])
    e_want = tangent(rng, angle)[0]
    Z = R.inv_se3(Xi) @ Xj @ R.inv_se3(R.exp_se3(e_want))     # so that the residual is e_want
    res = lambda A, B: R.log_se3(R.inv_se3(Z) @ R.inv_se3(A) @ B)
    e = res(Xi, Xj)
    assert np.abs(e - e_want).max() < 1e-12
    Jj = central(lambda d: res(Xi, Xj @ R.exp_se3(d)), h)
    Ji = central(lambda d: res(Xi @ R.exp_se3(d), Xj), h)
    assert np.abs(Jj - R.jr_inv(e)).max() < 1e-8
    assert np.abs(Ji + R.jr_inv(e) @ R.adjoint(R.inv_se3(Xj) @ Xi)).max() < 1e-8 * 10   # Ad carries |t| ~ 3
    assert np.abs(R.jr(e) @ R.jr_inv(e) - np.eye(6)).max() < 1e-13


def test_known_answer_straight_chain():
    """A straight chain along x with identity rotations and a Gaussian loop 0 -> n-1 whose length differs by D: weighted
    least squares in closed form, every odometry edge stretches by D s_o^2 / ((n-1) s_o^2 + s_l^2)."""
    n, D, var_l = 9, 0.3, 4e-4
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, 0, 3] = np.arange(n) * 1.0
    Z = np.eye(4)
    Z[0, 3] = (n - 1) * 1.0 + D
    g = R.build(poses, [(0, n - 1, Z, np.full(6, var_l), 0.0)])
    stretch = D * 1e-4 / ((n - 1) * 1e-4 + var_l)
    for solver in ("lstsq", "sparse"):
        X, info = g.optimize(solver=solver)
        assert info["converged"]
        assert np.abs(X[:, :3, :3] - np.eye(3)).max() < 1e-12
        assert np.abs(np.diff(X[:, 0, 3]) - (1.0 + stretch)).max() < 1e-10
        assert np.abs(X[:, 1:3, 3]).max() < 1e-12 and abs(X[0, 0, 3]) < 1e-12


def test_no_loops_returns_the_input():
    _, est, _ = S.circle(40)
    for solver in ("lstsq", "sparse"):
        X, info = R.build(est, []).optimize(solver=solver)
        assert info["converged"] and np.abs(X - est).max() < 1e-12


@pytest.fixture(scope="module")
def c24():
    true, est, loops = S.circle(24, loop_every=3, max_loops=4)
    g = R.build(est, loops)
    X, info = g.optimize(solver="lstsq")
    return g, est, X, info


def test_linear_solves_agree_at_200_nodes():
    """The QR solve of the whitened Jacobian against the sparse normal equations, one step at the drifted input of a
    200-node graph (cond(H) ~ 1e13: the normal equations lose up to cond * eps relative to the step's size)."""
    _, est, loops = S.circle(200)
    g = R.build(est, loops)
    a, b = g.gn_step_at(est, "lstsq"), g.gn_step_at(est, "sparse")
    assert np.abs(a).max() > 1e-3
    assert np.abs(a - b).max() < 1e-3 * np.abs(a).max() * 1e-3   # measured 1e-9 relative; cond * eps allows 1e-3


def test_restatement_converges_on_every_gpu_test_graph():
    """The convergence check the GPU tests apply to the device, applied to the restatement's own result first:
    the Gauss-Newton step at the returned poses is below 10 step_eps."""
    for true, est, loops in (S.circle(24, loop_every=3, max_loops=4), S.circle(65), S.hub(519)):
        g = R.build(est, loops)
        X, info = g.optimize(solver="sparse", step_eps=1e-10)
        assert info["converged"]
        assert np.abs(g.gn_step_at(X, "sparse")).max() < 10 * 1e-10


def test_cost_is_stationary_by_finite_differences(c24):
    """Central differences of cost() at the returned poses, per tangent coordinate, against the analytic gradient
    A^T r of the reweighted system (they are the same function only if weights and Jacobians are those of the robust
    cost) and against zero.  The finite-difference error is estimated from the differences themselves: truncation by
    Richardson from the step pair (h, 2h) (D(h) - D(2h)) / 3 is the leading h^2 term of D(h)), round-off
    eps cost / h per evaluation pair.  Zero is met up to the stopping rule: g = -H d with |d| < 10 step_eps."""
    g, est, X, info = c24
    n, h = len(X), 1e-4
    r, Ji, Jj, ei, ej = g.linearize(X)
    A = np.zeros((len(r), 6, n, 6))
    A[np.arange(len(r)), :, ej, :] = Jj
    A[np.arange(1, len(r)), :, ei[1:], :] = Ji[1:]
    A = A.reshape(6 * len(r), 6 * n)
    grad = A.T @ r.reshape(-1)
    Hm = A.T @ A
    Hrow, Hdiag = np.abs(Hm).sum(1), np.diag(Hm)
    cost = g.cost(X)
    u = 8 * EPS * (1 + np.abs(X[:, :3, 3]).max())
    scale = np.concatenate([1 / np.sqrt(g.prior_var)[None], np.sqrt(g._robust(g.residuals(X)[1])[1])[:, None] / np.sqrt(g._arrays()[3])], 0)
    rho = np.array([u * np.sum((np.abs(r) * scale)[(ei == k) | (ej == k)]) for k in range(n)])

    def diff(k, step):
        d = np.zeros((n, 6))
        d.reshape(-1)[k] = step
        return (g.cost(X @ R.exp_se3(d)) - g.cost(X @ R.exp_se3(-d))) / (2 * step)

    at_result = np.zeros(6 * n)
    for k in range(6 * n):
        d1, d2 = diff(k, h), diff(k, 2 * h)
        fd_err = 2 * abs(d1 - d2) / 3 + (rho[k // 6] + 2 * h * u * Hdiag[k] + 4 * EPS * (cost + 2 * h * h * Hdiag[k])) / h
        assert abs(d1 - grad[k]) <= fd_err + 1e-9 * abs(grad[k]), (k, d1, grad[k], fd_err)
        assert abs(d1) <= fd_err + Hrow[k] * 10 * 1e-10, (k, d1, fd_err)
        at_result[k] = d1
    # the same differences at the input, at a node a loop ends in, are far from zero: the check can fail
    node = g.ej[-1]
    at_input = []
    for k in range(6 * node, 6 * node + 6):
        d = np.zeros((n, 6))
        d.reshape(-1)[k] = h
        at_input.append((g.cost(est @ R.exp_se3(d)) - g.cost(est @ R.exp_se3(-d))) / (2 * h))
    assert np.abs(at_input).max() > 0.1 and np.abs(at_result[6 * node:6 * node + 6]).max() < 1e-3 * np.abs(at_input).max()


def test_robust_weights_and_cost():
    """Cauchy: w = k^2 / (k^2 + s), cost k^2/2 log(1 + s / k^2); k == 0 is Gaussian."""
    poses = np.tile(np.eye(4), (2, 1, 1))
    poses[1, 0, 3] = 1.0
    Z = np.eye(4)
    Z[0, 3] = 1.5                                  # e = (0, 0, 0, -0.5, 0, 0)
    for k, w, c in ((1.0, 1 / (1 + 2.5), 0.5 * np.log1p(2.5)), (2.0, 4 / (4 + 2.5), 2 * np.log1p(2.5 / 4)), (0.0, 1.0, 1.25)):
        g = R.build(poses, [(0, 1, Z, np.full(6, 0.1), k)])
        assert abs(g.weights(poses)[0] - w) < 4 * EPS and abs(g.cost(poses) - c) < 16 * EPS


def test_rpy_is_gtsams():
    from xchu_slam_amd import synth
    p = np.array([1.0, -2.0, 3.0, 0.3, -0.4, 2.9])
    assert np.abs(R.rpy(synth.pose_matrix(*p)) - p).max() < 8 * EPS * 3


# ------------------------------------------------------------------------------------------------ xa.loop_measurement
def test_loop_measurement_recovers_the_relative_pose():
    """T_icp corrects the current keyframe in the map frame: with T_icp = X_loop_est X_loop_true^-1 X_curr_true
    X_curr_est^-1 the default form gives Z = X_loop_true^-1 X_curr_true; the literal form gives T_icp^-1."""
    import xchu_slam_amd as xa
    true, est, accepted = S.drifted_route(sc_scene.route_poses())
    assert len(accepted) >= 10
    for loop, curr, T, _ in accepted:
        Z = xa.loop_measurement(est, loop, curr, T)
        assert np.abs(Z - R.inv_se3(true[loop]) @ true[curr]).max() < 256 * EPS * 30    # coordinates up to ~30 m
        lit = xa.loop_measurement(est, loop, curr, T, literal_measurement=True)
        assert np.abs(lit @ T - np.eye(4)).max() < 256 * EPS * 30
    # poses may be given as (x, y, z, roll, pitch, yaw)
    six = R.rpy(est)
    Z6 = xa.loop_measurement(six, accepted[0][0], accepted[0][1], accepted[0][2])
    assert np.abs(Z6 - xa.loop_measurement(est, *accepted[0][:3])).max() < 1e-12


def test_drifted_route_is_a_fair_input():
    """The input condition of the optimize_loops GPU test: the restatement's optimum has less than half of the drifted
    input's RMS position error against the truth."""
    import xchu_slam_amd as xa
    true, est, accepted = S.drifted_route(sc_scene.route_poses())
    loops = [(i, j, xa.loop_measurement(est, i, j, T), np.full(6, s), 1.0) for i, j, T, s in accepted]
    X, info = R.build(est, loops).optimize(solver="sparse")
    rms = lambda A: np.sqrt(((A - true)[:, :3, 3] ** 2).sum(1).mean())
    assert info["converged"] and rms(X) < 0.5 * rms(est), (rms(X), rms(est))
