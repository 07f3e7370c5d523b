#!/usr/bin/env python3
"""Times of pgo_node's Run loop (profiles/pgo_online.md): xa.PGO keyframe by keyframe against the batch path.

    python tools/pgo_online_profile.py                       # online "predict", online "optimize", batch; one JSON line
    python tools/pgo_online_profile.py --keyframes 300       # a prefix of the workload
    python tools/pgo_online_profile.py --solver direct --only predict    # PoseGraph's linear solver; one part alone

The workload: 1541 keyframes (the reference run's keyframe count) taken evenly from the KITTI-00 ground-truth trajectory
(tests/golden/kitti00_gt.npz, the selection of tools/pgo_profile.py and tools/globalmap_profile.py), each a synthetic
scan of N_POINTS points of one street world along that path (synth.make_street_world, so that a revisit sees the place
again) with a random intensity; the odometry is the truth drifted by tools/pgo_profile.py's seeded tangent noise (1e-3 rad
/ 1e-2 m per step).  Every pose is a keyframe (keyframe_gap -1), stamps are 1 s apart, the detector is Scan Context with
dist_thres 0.4 (the sparse synthetic scans need it, as in tests/test_gpu_scancontext.py) and the reference's period 30.

Online: PGO.push per keyframe with sync_timings, so that the wall time splits into store + descriptor, detection,
refinement and optimise (graph bookkeeping and read-back included); once with append="predict", once with "optimize".
Batch: the parent's path on the same input, close_loops(store=...) on the odometry and one optimize_loops.
ape is against the generating trajectory.  Times are host wall clock around calls that end synchronised.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KEYFRAMES, N_POINTS = 1541, 4000
DETECT = dict(dist_thres=0.4)
REFINE = dict(search_num=25, leaf=0.5)


def workload(n):
    import pgo_restate as R
    from xchu_slam_amd import synth
    from xchu_slam_amd.posegraph import _matrix_to_pose6d
    tum = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_gt.npz"))["tum"]
    sel = np.round(np.linspace(0, len(tum) - 1, N_KEYFRAMES)).astype(int)[:n]
    true = synth.kitti_poses(tum)[sel]
    rng = np.random.default_rng(7)
    est = [true[0]]
    for k in range(1, len(true)):
        noise = np.concatenate([rng.normal(size=3) * 1e-3, rng.normal(size=3) * 1e-2])
        est.append(est[-1] @ R.inv_se3(true[k - 1]) @ true[k] @ R.exp_se3(noise))
    odom = np.array([_matrix_to_pose6d(T) for T in est])
    xy = synth.kitti_poses(tum)[:, :2, 3]
    world = synth.make_street_world(11, xy, half=float(np.abs(xy).max() + 80.0))
    keyframes = []
    for i, T in enumerate(true):
        s = synth.sensor_scan(world, T, N_POINTS, 90_000 + i)
        keyframes.append(np.concatenate([s, np.random.default_rng(i).uniform(0, 1, (len(s), 1)).astype(np.float32)], 1))
    return true, odom, keyframes


def tum_rows(poses):
    """(n, 8) TUM rows, the index as the stamp, of (n, 4, 4) matrices or Pose6D rows."""
    from xchu_slam_amd.globalmap import _as_matrices, matrix_to_quaternion
    M = _as_matrices(poses)
    return np.array([[float(i), *m[:3, 3], *matrix_to_quaternion(m[:3, :3])] for i, m in enumerate(M)])


def errors(xa, poses, true):
    a, r = xa.ape(tum_rows(poses), tum_rows(true)), xa.rpe(tum_rows(poses), tum_rows(true))
    return {"ape_rmse_m": a["rmse"], "ape_max_m": a["max"], "rpe_rmse_m": r["rmse"]}


def online(xa, true, odom, keyframes, append, solver="cg"):
    with xa.PGO(keyframe_gap=-1.0, detect_args=DETECT, append=append, solver=solver, **REFINE) as pgo:
        pgo.sync_timings = True
        pgo.keep_poses_before = False
        split = dict.fromkeys(("store", "detect", "refine", "optimize"), 0.0)
        worst, solve_ms = 0.0, []
        t0 = time.perf_counter()
        for k, (cloud, pose) in enumerate(zip(keyframes, odom)):
            t1 = time.perf_counter()
            rec = pgo.push(cloud, pose, float(k))
            worst = max(worst, time.perf_counter() - t1)
            for name, ms in rec["ms"].items():
                split[name] += ms
            if rec["info"]:
                solve_ms.append(rec["ms"]["optimize"])
            if k % 200 == 199:
                print(f"{append}: {k + 1} keyframes, {time.perf_counter() - t0:.1f} s, {len(pgo.loops)} loops", file=sys.stderr, flush=True)
        total = time.perf_counter() - t0
        solves = [r["info"] for r in pgo.log if r["info"]]
        out = {"append": append, "solver": solver, "ms_mean_solve": float(np.mean(solve_ms)) if solve_ms else 0.0,
               "ms_worst_solve": max(solve_ms, default=0.0), "d_last": pgo._graph.solver_stats()["d"], "s_total": total, "ms_per_keyframe": 1e3 * total / len(odom), "ms_worst_keyframe": 1e3 * worst,
               "s_split": {k: v / 1e3 for k, v in split.items()}, "candidates": sum(1 for r in pgo.log if r["candidate"] != -1),
               "refined": sum(1 for r in pgo.log if r["refined"]), "accepted": len(pgo.loops),
               "gate_rejected": sum(1 for r in pgo.rejected if r[2] == "pair_distance"),
               "optimize_launches": pgo.optimize_launches, "cg_iterations": pgo.cg_iterations,
               "outer_iterations": sum(i["iterations"] for i in solves), "not_converged": sum(1 for i in solves if not i["converged"])}
        out.update(errors(xa, pgo.poses, true))
        return out


def batch(xa, true, odom, keyframes, solver="cg"):
    from xchu_slam_amd import synth
    from xchu_slam_amd.posegraph import _matrix_to_pose6d
    with xa.KeyframeMap() as store:
        t0 = time.perf_counter()
        for k in keyframes:
            store.add(k)
        t_store = time.perf_counter() - t0
        t0 = time.perf_counter()
        accepted, rejected = xa.close_loops(None, [tuple(p) for p in odom], detect_args=dict(DETECT, tree_making_period=30), store=store, **REFINE)
        t_close = time.perf_counter() - t0
        # optimize_loops hands the f32 ICP transform to the graph as it is, and the graph refuses a measurement whose
        # rotation is further than 1e-6 from orthonormal, which an f32 product of many ICP steps can be: counted, then
        # every transform goes through Matrix2Pose6D / Pose6D2Matrix as xa.PGO does
        raw = [np.asarray(T, np.float64)[:3, :3] for _, _, T, _ in accepted]
        not_rigid = sum(1 for Rm in raw if np.abs(Rm.T @ Rm - np.eye(3)).max() > 1e-6)
        accepted = [(i, j, synth.pose_matrix(*_matrix_to_pose6d(np.asarray(T, np.float64))), s) for i, j, T, s in accepted]
        t0 = time.perf_counter()
        poses, info = xa.optimize_loops(odom, accepted, registration=store.registration, solver=solver)
        t_opt = time.perf_counter() - t0
    out = {"solver": solver, "s_store": t_store, "s_close_loops": t_close, "s_optimize_loops": t_opt, "s_total": t_store + t_close + t_opt,
           "accepted": len(accepted), "transforms_not_rigid_to_1e-6": not_rigid, "rejected_icp": sum(1 for r in rejected if r[2] == "icp"),
           "gate_rejected": sum(1 for r in rejected if r[2] == "pair_distance"), "iterations": info["iterations"],
           "converged": info["converged"], "cg_iterations": info["cg_iterations"]}
    out.update(errors(xa, poses, true))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=N_KEYFRAMES)
    ap.add_argument("--solver", default="cg", help="PoseGraph's linear solver: cg, direct, or both (each part run with cg, then direct)")
    ap.add_argument("--only", default="", help="comma-separated parts to run (predict, optimize, batch); default: all three")
    a = ap.parse_args()
    import xchu_slam_amd as xa
    t0 = time.perf_counter()
    true, odom, keyframes = workload(a.keyframes)
    res = {"keyframes": len(odom), "points_per_keyframe": N_POINTS, "s_generate": time.perf_counter() - t0,
           "odometry": errors(xa, odom, true)}
    parts = {"predict": lambda sv: online(xa, true, odom, keyframes, "predict", sv),
             "optimize": lambda sv: online(xa, true, odom, keyframes, "optimize", sv),
             "batch": lambda sv: batch(xa, true, odom, keyframes, sv)}
    for name in (a.only.split(",") if a.only else parts):
        for sv in (("cg", "direct") if a.solver == "both" else (a.solver,)):
            key = name if a.solver != "both" else f"{name}_{sv}"
            while key in res:        # a part named twice (--only predict,predict) runs twice, alternating the solvers
                key += "+"
            res[key] = parts[name](sv)
            print(key, json.dumps(res[key]), file=sys.stderr, flush=True)      # each part as it finishes
    print(json.dumps(res))
