"""Synthetic pose graphs of the pose-graph tests: a circle driven for two laps with drifted odometry and a loop to the
first lap every few keyframes, a graph with a hub node, and a drifted copy of the Scan Context route."""
import math

import numpy as np

import pgo_restate as R


def circle(n, laps=2.0, radius=20.0, seed=1, drift=(2e-3, 2e-2), loop_every=5, loop_noise=0.02, fitness=0.1, max_loops=None):
    """(true (n, 4, 4), drifted (n, 4, 4), loops [(i, j, Z, var, k)]): n keyframes over `laps` laps; the drifted poses
    compose the true relative poses with a tangent noise of (rad, m) `drift` per step; from the second lap on every
    loop_every-th keyframe j closes on the keyframe i one lap earlier, measured with tangent noise loop_noise."""
    rng = np.random.default_rng(seed)
    per = n / laps
    true = []
    for k in range(n):
        a = 2 * math.pi * k / per
        T = np.eye(4)
        T[:3, :3] = R.exp_se3(np.array([0.02 * math.sin(3 * a), 0.03 * math.cos(2 * a), a + math.pi / 2, 0, 0, 0]))[:3, :3]
        T[:3, 3] = [radius * math.cos(a), radius * math.sin(a), 0.5 * math.sin(a)]
        true.append(T)
    true = np.array(true)
    est = [true[0]]
    for k in range(1, n):
        noise = np.concatenate([rng.normal(size=3) * drift[0], rng.normal(size=3) * drift[1]])
        est.append(est[-1] @ R.inv_se3(true[k - 1]) @ true[k] @ R.exp_se3(noise))
    est = np.array(est)
    loops, lap = [], int(round(per))
    for j in range(lap, n, loop_every):
        if max_loops is not None and len(loops) >= max_loops:
            break
        i = j - lap
        loops.append((i, j, R.inv_se3(true[i]) @ true[j] @ R.exp_se3(rng.normal(size=6) * loop_noise), np.full(6, fitness), 1.0))
    return true, est, loops


def hub(n, hub_node=10, hub_edges=70, seed=2):
    """A circle graph plus hub_edges loops that all end in hub_node (alternately as i and as j)."""
    true, est, loops = circle(n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    others = [k for k in range(n) if abs(k - hub_node) > 1]
    for q, k in enumerate(rng.choice(others, hub_edges, replace=False)):
        i, j = (hub_node, int(k)) if q % 2 else (int(k), hub_node)
        loops.append((i, j, R.inv_se3(true[i]) @ true[j] @ R.exp_se3(rng.normal(size=6) * 0.02), np.full(6, 0.2), 1.0))
    return true, est, loops


def drifted_route(poses6, seed=4, drift=(1.5e-3, 1.5e-2), score=0.01):
    """The Scan Context route (sc_scene.route_poses) with drifted odometry and the `accepted` records close_loops would
    return for its revisits, built from the truth: T_icp = X_loop_est X_loop_true^-1 X_curr_true X_curr_est^-1 (the
    correction of the current keyframe in the map frame), every second revisit.  Returns (true, est, accepted)."""
    from xchu_slam_amd import synth
    rng = np.random.default_rng(seed)
    true = np.array([synth.pose_matrix(*p) for p in poses6])
    est = [true[0]]
    for k in range(1, len(true)):
        noise = np.concatenate([rng.normal(size=3) * drift[0], rng.normal(size=3) * drift[1]])
        est.append(est[-1] @ R.inv_se3(true[k - 1]) @ true[k] @ R.exp_se3(noise))
    est = np.array(est)
    accepted = []
    for curr in range(79, len(true), 2):
        loop = curr - 79
        T = est[loop] @ R.inv_se3(true[loop]) @ true[curr] @ R.inv_se3(est[curr])
        accepted.append((loop, curr, T, score))
    return true, est, accepted
