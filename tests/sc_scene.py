"""The loop route of the Scan Context tests: a 25 m-radius circle driven for 1.3 laps with a keyframe every 2 m
(102 keyframes; from keyframe ~79 on, the place of keyframe q - 79 is seen again, 0.9 m further along)."""
import math

import numpy as np

from xchu_slam_amd import synth

RADIUS, SPACING, LAPS = 25.0, 2.0, 1.3
HEIGHT = 1.73


def route_poses():
    """(x, y, z, roll, pitch, yaw) per keyframe, heading along the circle."""
    n = int(LAPS * 2 * math.pi * RADIUS / SPACING)
    out = []
    for i in range(n):
        a = i * SPACING / RADIUS
        yaw = a + math.pi / 2
        out.append((RADIUS * math.cos(a), RADIUS * math.sin(a), HEIGHT, 0.0, 0.0, math.atan2(math.sin(yaw), math.cos(yaw))))
    return out


def route_world(seed=5):
    poses = route_poses()
    xy = np.array([[p[0], p[1]] for p in poses])
    return synth.make_street_world(seed, xy, half=110.0)


def route_keyframes(n_points=3000, seed=5, max_range=60.0):
    """(keyframes [(n_points, 3) f32, sensor frame], poses)."""
    poses = route_poses()
    world = route_world(seed)
    scans = [synth.sensor_scan(world, synth.pose_matrix(*p), n_points, 1000 * seed + i, max_range=max_range)
             for i, p in enumerate(poses)]
    return scans, poses
