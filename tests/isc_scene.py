"""The loop route of the Intensity Scan Context tests: sc_scene's route (102 keyframes, 3000 points each, seed 5) with a
reflectance per point that depends on the place alone, so that a revisit sees the intensities of the first visit.

The world point (pose . p, f64) falls in a 4 m cell c = floor(pw / 4); the cell's hash
h = (cx * 73856093) ^ (cy * 19349663) ^ (cz * 83492791) (int64) gives intensity = f32((h mod 200) + 30) / f32(255), inside
the detector's 0..1 contract.  `yaw_offset` turns the sensor by that angle from keyframe 60 on: a scan depends on the
sensor's position only, so this rotates the sensor-frame cloud of the revisiting keyframes against the first lap's."""
import math

import numpy as np

import sc_scene
from xchu_slam_amd import synth

YAW_FROM = 60
CELL = 4.0


def reflectance(world_pts: np.ndarray) -> np.ndarray:
    c = np.floor(np.asarray(world_pts, np.float64) / CELL).astype(np.int64)
    h = (c[:, 0] * 73856093) ^ (c[:, 1] * 19349663) ^ (c[:, 2] * 83492791)
    return ((h % 200) + 30).astype(np.float32) / np.float32(255)


def route_poses(yaw_offset: float = 0.0):
    out = []
    for i, p in enumerate(sc_scene.route_poses()):
        yaw = p[5] + (yaw_offset if i >= YAW_FROM else 0.0)
        out.append(p[:5] + (math.atan2(math.sin(yaw), math.cos(yaw)),))
    return out


def route_keyframes(n_points=3000, seed=5, yaw_offset: float = 0.0, max_range=60.0):
    """(keyframes [(n_points, 4) f32 x,y,z,intensity, sensor frame], poses)."""
    poses = route_poses(yaw_offset)
    world = sc_scene.route_world(seed)
    out = []
    for i, p in enumerate(poses):
        T = synth.pose_matrix(*p)
        scan = synth.sensor_scan(world, T, n_points, 1000 * seed + i, max_range=max_range)
        pw = scan.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        out.append(np.concatenate([scan, reflectance(pw)[:, None]], 1).astype(np.float32))
    return out, poses
