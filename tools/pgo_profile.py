#!/usr/bin/env python3
"""Times of the pose-graph optimiser (profiles/posegraph.md): one ndt_pgo_optimize of a KITTI-00-shaped graph.

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python tools/pgo_profile.py   # the workload, traced
    python tools/pgo_profile.py --summarise DIR/run_kernel_trace.csv                             # kernel times
    python tools/pgo_profile.py --restatement                                                    # tests/pgo_restate.py, no GPU
    python tools/pgo_profile.py --altitude                          # the workload with a position factor on every keyframe

The graph: 1541 keyframes (the reference run's keyframe count) taken evenly from the KITTI-00 ground-truth trajectory
(tests/golden/kitti00_gt.npz), odometry drifted by a seeded tangent noise of 1e-3 rad / 1e-2 m per step (one sigma of
odomNoise), and a loop from every REVISIT_EVERY-th keyframe that comes within 5 m of a keyframe at least 200 keyframes
older, measured from the truth with 0.02 tangent noise and variance 0.1 (an ICP fitness score), Cauchy k = 1.

The workload optimises the same graph WARMUP + REPEATS times (each from the drifted input) and prints one JSON line with
the host wall time of the call and the optimiser's own record; --summarise reads k_pgo_optimize's dispatches out of the
trace.  --restatement times tests/pgo_restate.py (sparse normal equations) on the same graph, for scale.
--altitude (profiles/posegraph_gps.md) adds pgo_node's GPS factor to every keyframe: its own x and y with variance 1e9,
the true altitude with variance 250, Cauchy k = 1.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KEYFRAMES, WARMUP, REPEATS, REVISIT_EVERY = 1541, 2, 10, 2


def quat_pose(row):
    _, x, y, z, qx, qy, qz, qw = row
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                 [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                 [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
    T[:3, 3] = [x, y, z]
    return T


def graph():
    import pgo_restate as R
    tum = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_gt.npz"))["tum"]
    rows = tum[np.round(np.linspace(0, len(tum) - 1, N_KEYFRAMES)).astype(int)]
    rows[:, 4:] /= np.linalg.norm(rows[:, 4:], axis=1, keepdims=True)
    true = np.array([quat_pose(r) for r in rows])
    rng = np.random.default_rng(7)
    est = [true[0]]
    for k in range(1, len(true)):
        noise = np.concatenate([rng.normal(size=3) * 1e-3, rng.normal(size=3) * 1e-2])
        est.append(est[-1] @ R.inv_se3(true[k - 1]) @ true[k] @ R.exp_se3(noise))
    est = np.array(est)
    xyz = true[:, :3, 3]
    loops, seen = [], 0
    for j in range(201, len(true)):
        d = np.linalg.norm(xyz[:j - 200] - xyz[j], axis=1)
        i = int(np.argmin(d))
        if d[i] > 5.0:
            continue
        seen += 1
        if seen % REVISIT_EVERY:
            continue
        loops.append((i, j, R.inv_se3(true[i]) @ true[j] @ R.exp_se3(rng.normal(size=6) * 0.02), np.full(6, 0.1), 1.0))
    return true, est, loops


def rms(A, B):
    return float(np.sqrt(((A - B)[:, :3, 3] ** 2).sum(1).mean()))


def device(altitude=False, solver="cg"):
    import xchu_slam_amd as xa
    true, est, loops = graph()
    wall, info, hist, X, stats = [], None, None, None, None
    for _ in range(WARMUP + REPEATS):
        with xa.PoseGraph(solver=solver) as pg:
            for P in est:
                pg.add_node(P)
            for i, j, Z, var, k in loops:
                pg.add_loop(i, j, Z, var, k)
            if altitude:
                for k in range(len(est)):
                    pg.add_position(k, [est[k, 0, 3], est[k, 1, 3], true[k, 2, 3]], [1e9, 1e9, 250.0], 1.0)
            t0 = time.perf_counter()
            info = pg.optimize()
            wall.append((time.perf_counter() - t0) * 1e3)
            hist, X, stats = pg.history(), pg.poses(), pg.solver_stats()
    print(json.dumps({"solver": stats, "ms_per_outer_iteration": float(statistics.median(wall[WARMUP:])) / max(1, info["iterations"]), "nodes": len(est), "loops": len(loops), "positions": len(est) if altitude else 0, "ms_wall_call": float(statistics.median(wall[WARMUP:])), "info": info,
                      "cg_per_iteration": [r["cg_iterations"] for r in hist], "rms_in_m": rms(est, true), "rms_out_m": rms(X, true),
                      "z_rms_in_m": float(np.sqrt(((est - true)[:, 2, 3] ** 2).mean())), "z_rms_out_m": float(np.sqrt(((X - true)[:, 2, 3] ** 2).mean()))}))


def summarise(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    v = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if "k_pgo_optimize" in r["Kernel_Name"]]
    if v:
        assert len(v) == WARMUP + REPEATS, len(v)
        v = v[WARMUP:]
        print(f"k_pgo_optimize  n {len(v)}  median {statistics.median(v):.3f} ms  min {min(v):.3f}  max {max(v):.3f}")
    # the direct solve's kernels: dispatches and device time summed over the whole run (WARMUP + REPEATS optimises)
    per = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        if name.startswith(("k_pgo_direct", "k_pgo_schur", "k_pgo_chol")):
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in per.items():
        print(f"{name}  n {len(us)}  total {sum(us) / 1e3:.3f} ms  median {statistics.median(us):.2f} us  max {max(us):.2f} us")


def restatement():
    import pgo_restate as R
    true, est, loops = graph()
    g = R.build(est, loops)
    t0 = time.perf_counter()
    X, info = g.optimize(solver="sparse", step_eps=1e-10, max_iter=200)
    info.pop("history")
    print(json.dumps({"nodes": len(est), "loops": len(loops), "s_wall": time.perf_counter() - t0, "info": info, "rms_in_m": rms(est, true),
                      "rms_out_m": rms(X, true), "threads": os.environ.get("OMP_NUM_THREADS", "")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--altitude", action="store_true")
    ap.add_argument("--solver", default="cg", choices=("cg", "direct"), help="PoseGraph's linear solver")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", default="")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    elif a.restatement:
        restatement()
    else:
        device(a.altitude, a.solver)
