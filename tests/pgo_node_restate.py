"""Restatement of the host rules of pgo_node's Run loop (xchu_mapping/src/pgo_node.cpp), in plain Python, and hand cases
for them.  No GPU, no package import.

keyframe_gate    :188-205 with pgo.h:96,136: f64; the previous pose starts at (0, 0, 0), the accumulator at 1 000 000;
                 the step is between consecutive received poses; a keyframe needs accumulated > gap (strict) and resets
                 the accumulator.
radius_candidate :300-327 (loop_method 0): nothing below 30 keyframes; candidates are all stored keyframes (the current
                 one included) whose f32 planar squared distance to the current corrected pose is below 20^2; ascending
                 squared distance; the first whose time differs from the current keyframe's by more than 30.0 s (strict).
radius_accept    :328-341: the planar distance of the corrected poses (f64) must be below 30.0.
FLANN is not in the reference tree: the strictness of the radius test and the order of equal distances (lower index first)
are modelled.
"""
import math

import numpy as np


def keyframe_gate(positions, gap=2.0):
    prev = (0.0, 0.0, 0.0)
    acc = 1000000.0
    out = []
    for k, p in enumerate(positions):
        cur = (float(p[0]), float(p[1]), float(p[2]))
        acc += math.sqrt((prev[0] - cur[0]) ** 2 + (prev[1] - cur[1]) ** 2 + (prev[2] - cur[2]) ** 2)
        prev = cur
        if acc > gap:
            out.append(k)
            acc = 0.0
    return out


def radius_candidate(poses, times, min_keyframes=30, radius=20.0, min_time_gap=30.0):
    n = len(poses)
    if n < min_keyframes:
        return -1
    f = np.float32
    cx, cy = f(poses[n - 1][0]), f(poses[n - 1][1])
    found = []
    for i in range(n):
        dx, dy = f(poses[i][0]) - cx, f(poses[i][1]) - cy
        d2 = f(f(dx * dx) + f(dy * dy))
        if d2 < f(radius) * f(radius):
            found.append((d2, i))
    found.sort()                       # ascending distance, then ascending index
    for _, i in found:
        if abs(times[i] - times[n - 1]) > min_time_gap:
            return i
    return -1


def radius_accept(poses, prev, curr, limit=30.0):
    return math.sqrt((poses[prev][0] - poses[curr][0]) ** 2 + (poses[prev][1] - poses[curr][1]) ** 2) < limit


def line(n, spacing=1.0, dt=2.0):
    """n keyframes along +x, `spacing` metres and `dt` seconds apart: (poses (n, 6), times)."""
    poses = np.zeros((n, 6))
    poses[:, 0] = spacing * np.arange(n)
    return poses, dt * np.arange(n)


def hand_cases():
    """[(name, poses, times, expected candidate)] for radius_candidate."""
    cases = []
    # 40 keyframes out along x, 2 s apart; the last one is placed by hand.  Keyframes 0..23 are more than 30 s old.
    poses, times = line(40)
    poses[39, :2] = [10.2, 0.5]                     # nearest old keyframe: 10 (d2 0.29), then 11, 9, ...
    cases.append(("nearest first", poses.copy(), times.copy(), 10))
    poses[39, :2] = [23.6, 0.0]                     # 24 is nearer (0.4 m) but exactly 30 s old; 23 (0.6 m) is 32 s old
    cases.append(("the nearest is too young", poses.copy(), times.copy(), 23))
    # 30 s strict: the only keyframe in range is exactly 30.0 s older -> not chosen; 30.0 + a little -> chosen
    poses, times = line(31, spacing=100.0, dt=1.0)
    poses[30, :2] = poses[0, :2] + [1.0, 0.0]
    times[30] = times[0] + 30.0
    cases.append(("30 s is not enough", poses.copy(), times.copy(), -1))
    times[30] = np.nextafter(times[0] + 30.0, 100.0)
    cases.append(("just over 30 s", poses.copy(), times.copy(), 0))
    # the current keyframe is the nearest of all (distance 0) and never chosen: its time difference is 0
    poses, times = line(35, spacing=100.0, dt=10.0)
    cases.append(("the current keyframe alone in range", poses.copy(), times.copy(), -1))
    # radius strict: f32 squared distance exactly 400 is out, the f32 below 20 m is in
    poses, times = line(32, spacing=100.0, dt=10.0)
    poses[31, :2] = poses[3, :2] + [20.0, 0.0]
    cases.append(("exactly 20 m", poses.copy(), times.copy(), -1))
    poses[31, :2] = poses[3, :2] + [0.0, float(np.nextafter(np.float32(20.0), np.float32(0.0)))]
    cases.append(("just under 20 m", poses.copy(), times.copy(), 3))
    poses[31, :2] = poses[3, :2] + [12.0, 16.0]    # 144 + 256 = 400 exactly in f32
    cases.append(("3-4-5 at exactly 20 m", poses.copy(), times.copy(), -1))
    # equal distances: keyframes 5 and 2 are both 3 m from the current one -> the lower index
    poses, times = line(33, spacing=100.0, dt=10.0)
    poses[5, :2] = [1050.0, 3.0]
    poses[2, :2] = [1053.0, 0.0]
    poses[32, :2] = [1050.0, 0.0]
    cases.append(("equal distances", poses.copy(), times.copy(), 2))
    # fewer than 30 keyframes: nothing, though keyframe 0 is 1 m away and 56 s old; with the 30th it is found
    poses, times = line(29, spacing=100.0, dt=2.0)
    poses[28, :2] = [1.0, 0.0]
    cases.append(("29 keyframes", poses.copy(), times.copy(), -1))
    poses, times = line(30, spacing=100.0, dt=2.0)
    poses[29, :2] = [1.0, 0.0]
    cases.append(("30 keyframes", poses.copy(), times.copy(), 0))
    return cases
