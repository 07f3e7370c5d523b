"""The graphs of the position-factor tests (tests/test_pgo_position_restate.py on the CPU, tests/test_gpu_pgo_position.py on
the device): tests/pgo_scene.py's circles, hub graph and drifted route with position factors [(node, xyz, var, k)] whose
measurements are taken from the true poses.  Each returns (true, est, loops, positions)."""
import numpy as np

import pgo_scene as S

ALT_VAR = (1e9, 1e9, 250.0)     # pgo_node.cpp:104-108: x and y free, altitude 250
TIGHT_VAR = (1e-2, 1e-2, 1e-2)
THREADS = 512                   # ndt::kPgoBlock


def altitude(true, est, nodes, k=1.0):
    """pgo_node's constraint (pgo_node.cpp:283): the keyframe's own x and y, the measured (here: true) altitude."""
    return [(int(n), np.array([est[n, 0, 3], est[n, 1, 3], true[n, 2, 3]]), np.array(ALT_VAR), k) for n in nodes]


def chain():
    """A 40-node chain with no loops, an altitude factor on every 5th node."""
    true, est, _ = S.circle(40)
    return true, est, [], altitude(true, est, range(0, 40, 5))


def circle():
    """circle(65) with its 7 loops; altitude factors on node 0 (under the prior), 63 and 64 (either side of the wave
    boundary; 64 is the last node) and a few between, two of them on node 20."""
    true, est, loops = S.circle(65)
    pos = altitude(true, est, [0, 20, 33, 63, 20, 64, 7])
    pos[4][1][2] += 0.3      # the second factor of node 20 disagrees with the first
    return true, est, loops, pos


def hub():
    """hub(519) with an altitude factor on every node and a second one on the hub node: more factors than the workgroup
    has threads, runs of two nodes per thread in the scans, and one gather of 70 edges and 2 position factors."""
    true, est, loops = S.hub(THREADS + 7)
    return true, est, loops, altitude(true, est, list(range(THREADS + 7)) + [10])


def tight():
    """circle(65) without loops, the true position with variance 1e-2 on all three axes on every 8th node: the optimum
    is pulled off the drifted odometry by decimetres in x, y and z (a wrong sign or transpose in K shows here)."""
    true, est, _ = S.circle(65)
    return true, est, [], [(n, true[n, :3, 3].copy(), np.array(TIGHT_VAR), 1.0) for n in range(0, 65, 8)]


def gaussian():
    """circle() with the factor on node 33 Gaussian (k = 0)."""
    true, est, loops, pos = circle()
    pos[2] = pos[2][:3] + (0.0,)
    return true, est, loops, pos


def outlier():
    """circle() with the altitude of node 33 500 m off."""
    true, est, loops, pos = circle()
    pos[2][1][2] += 500.0
    return true, est, loops, pos


def route(altitude_var=1e-2):
    """The drifted Scan Context route (pgo_scene.drifted_route) moved down so that its first keyframe is at altitude 0,
    which is what pgo_node's offset assumes; keyframes every 0.5 s, a fix 0.03 s after every third one whose altitude is
    the true z plus 120 m, turned into factors by xa.gps_factors.  altitude_var is 1e-2, a 0.1 m altimeter: at pgo_node's
    250 the factors are so weak against the odometry (variance 1e-4 per step) that the optimum's z-RMS moves from
    0.09126 m to 0.09120 m; at 1e-2 it falls to 0.0334 m.  Returns (true, est, loops, positions, accepted)."""
    import sc_scene
    import xchu_slam_amd as xa
    p6 = np.array(sc_scene.route_poses(), np.float64)
    p6[:, 2] -= p6[0, 2]
    true, est, accepted = S.drifted_route(p6)
    loops = [(i, j, xa.loop_measurement(est, i, j, T), np.full(6, s), 1.0) for i, j, T, s in accepted]
    kt = 10.0 + 0.5 * np.arange(len(est))
    sel = np.arange(0, len(est), 3)
    pos = gps(est, kt, kt[sel] + 0.03, 120.0 + true[sel, 2, 3], altitude_var)
    return true, est, loops, [p + (1.0,) for p in pos], accepted


def gps(est, kt, gt, alt, altitude_var=1e-2):
    import xchu_slam_amd as xa
    return xa.gps_factors(kt, est, gt, alt, altitude_var=altitude_var)


# the restatement's spread per graph class (tests/test_pgo_position_restate.py measures it; the figures are in
# tests/test_gpu_pgo_position.py's docstring)
CLASSES = {"circle": (chain, circle, gaussian, outlier), "tight": (tight,), "hub": (hub,), "route": (route,)}
SPREAD = {"circle": 1.15e-11, "tight": 2.82e-11, "hub": 3.27e-11, "route": 4.08e-11}
