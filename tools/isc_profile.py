#!/usr/bin/env python3
"""Times of the Intensity Scan Context path (profiles/isc.md): k_isc_make next to k_sc_make on one 120 k-point scan, one
ndt_isc_detect against 1541 keyframes placed along the KITTI-00 trajectory, one ndt_isc_detect_batch over all 1541.

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python tools/isc_profile.py   # the workload, traced
    python tools/isc_profile.py --summarise DIR/run_kernel_trace.csv                             # kernel times
    python tools/isc_profile.py --restatement [--jobs 16]                                        # tests/isc_restate.py, no GPU

The workload runs its cases in a fixed order (WARMUP + REPEATS adds of the big scan to a Scan Context and to an ISC
database, the 1541 keyframe adds, WARMUP + REPEATS single detections, 1 + BATCH_REPEATS batches) and prints the host wall
time of each call as one JSON line; --summarise picks each case's dispatches out of the trace by that order.
--restatement times the numpy restatement on the same inputs, the batch spread over --jobs processes (Python on the host,
for scale only).

The 1541 keyframes stand at every third pose or so of tests/golden/kitti00_gt.npz (3724 m, with its revisits), at (x, y, 0)
as pgo_node passes them.  Their clouds are seeded: 3000 points on 24 wall segments within 40 m, so that a descriptor is
sparse, as a street scan's is; then every gated pair passes the geometry threshold and runs the 20 intensity shifts too —
the costliest case for k_isc_detect.
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KEYFRAMES, N_SCAN, WARMUP, REPEATS, BATCH_REPEATS = 1541, 120_000, 3, 20, 5


def keyframe(i, n=3000, walls=24):
    rng = np.random.default_rng(50_000 + i)
    a = rng.uniform(-38, 38, (walls, 2))
    b = a + rng.uniform(-12, 12, (walls, 2))
    w = rng.integers(0, walls, n)
    t = rng.uniform(0, 1, n)[:, None]
    xy = a[w] * (1 - t) + b[w] * t + rng.normal(0, 0.03, (n, 2))
    return np.concatenate([xy, rng.uniform(-0.5, 8.0, (n, 1)), rng.uniform(0.1, 0.9, (n, 1))], 1).astype(np.float32)


def positions():
    from xchu_slam_amd import synth
    tum = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_gt.npz"))["tum"]
    sel = np.round(np.linspace(0, len(tum) - 1, N_KEYFRAMES)).astype(int)
    poses = synth.kitti_poses(tum)[sel]
    return [(float(p[0, 3]), float(p[1, 3]), 0.0) for p in poses]


def big_scan():
    from xchu_slam_amd import synth
    world = synth.make_world(3, half=110.0)
    xyz = synth.sensor_scan(world, synth.pose_matrix(0.0, 0.0, 1.73, 0.0, 0.0, 0.3), N_SCAN, 11, max_range=80.0)
    w = np.random.default_rng(12).uniform(0, 1, (len(xyz), 1))
    return np.concatenate([xyz, w], 1).astype(np.float32)


def med(v):
    return float(statistics.median(v))


def synced_call(obj, f):
    """Host wall time (ms) of f() followed by a synchronise of the context."""
    t0 = time.perf_counter()
    out = f()
    assert obj._lib.ndt_synchronize(obj.ctx) == 0
    return (time.perf_counter() - t0) * 1e3, out


def device():
    import xchu_slam_amd as xa
    res = {}
    scan = big_scan()
    with xa.SCManager(tree_making_period=1) as sc, xa.ISCGeneration(registration=sc.registration) as isc:
        lib, ctx = sc._lib, sc.ctx
        d = C.c_void_p()
        assert lib.ndt_device_alloc(ctx, scan.nbytes, C.byref(d)) == 0
        assert lib.ndt_memcpy_h2d(ctx, d, scan.ctypes.data_as(C.c_void_p), scan.nbytes) == 0
        wall_sc = [synced_call(sc, lambda: sc.makeAndSaveScancontextAndKeysDevice(d.value, len(scan)))[0]
                   for _ in range(WARMUP + REPEATS)][WARMUP:]
        wall = [synced_call(isc, lambda: isc.makeAndSavedecDevice(d.value, len(scan), (0, 0, 0)))[0]
                for _ in range(WARMUP + REPEATS)][WARMUP:]
        lib.ndt_device_free(ctx, d)
        res["make_120k"] = {"ms_wall_call": med(wall), "ms_wall_call_sc": med(wall_sc), "points": len(scan), "bytes_read": scan.nbytes,
                            "cells_filled": int(np.count_nonzero(isc.getLastISCMONO()))}
    pos = positions()
    with xa.ISCGeneration() as isc:
        for i in range(N_KEYFRAMES):
            isc.makeAndSavedec(keyframe(i), pos[i])
        wall = [synced_call(isc, isc.detectLoopClosureID)[0] for _ in range(WARMUP + REPEATS)][WARMUP:]
        res["detect_one"] = {"ms_wall_call": med(wall), "stored": len(isc), "record": isc.last_result()}
        query = np.arange(len(isc))
        runs = [synced_call(isc, lambda: isc.detect_batch(query)) for _ in range(1 + BATCH_REPEATS)][1:]
        recs = runs[-1][1]
        res["detect_batch"] = {"ms_wall_call": med([w for w, _ in runs]), "queries": len(query),
                               "gated_pairs": int(sum(r["n_gated"] for r in recs)), "geometry_pairs": int(sum(r["n_geometry"] for r in recs)),
                               "loop_pairs": int(sum(r["n_loop_pairs"] for r in recs)), "loops": int(sum(r["loop_id"] != -1 for r in recs)),
                               "last": recs[-1]}
    print(json.dumps(res))


def summarise(path):
    """Kernel times out of a rocprofv3 kernel trace of device(), by the order of the dispatches."""
    by = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("ndt::", "")
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    big = WARMUP + REPEATS
    assert len(by["k_sc_make"]) == big and len(by["k_isc_make"]) == big + N_KEYFRAMES, {k: len(v) for k, v in by.items()}
    assert len(by["k_isc_detect"]) == len(by["k_isc_reduce"]) == big + 1 + BATCH_REPEATS, len(by["k_isc_detect"])
    cases = {"k_sc_make, 120k points": by["k_sc_make"][WARMUP:big], "k_isc_make, 120k points": by["k_isc_make"][WARMUP:big],
             "k_isc_finalize": by["k_isc_finalize"][WARMUP:big], "k_isc_make, 3000 points": by["k_isc_make"][big:],
             "k_isc_detect, one query": by["k_isc_detect"][WARMUP:big], "k_isc_reduce, one query": by["k_isc_reduce"][WARMUP:big],
             "k_isc_detect, batch": by["k_isc_detect"][big + 1:], "k_isc_reduce, batch": by["k_isc_reduce"][big + 1:]}
    for name, v in cases.items():
        print(f"{name:28s} n {len(v):5d}  median {med(v):8.2f} us  min {min(v):8.2f}  max {max(v):8.2f}")


_G = None


def _detect(q):
    return _G.detect(q)


def restatement(jobs):
    import multiprocessing as mp
    import isc_restate as R
    global _G
    res = {"jobs": jobs}
    scan = big_scan()
    t0 = time.perf_counter()
    R.calculate_isc(scan)
    res["make_120k_s"] = time.perf_counter() - t0
    pos = positions()
    g = R.ISCGeneration()
    g.cache = None
    for i in range(N_KEYFRAMES):
        g.makeAndSavedec(keyframe(i), pos[i])
    t0 = time.perf_counter()
    rec = g.detect(N_KEYFRAMES - 1)
    res["detect_one_s"] = time.perf_counter() - t0
    res["detect_one_record"] = rec
    _G = g
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(jobs) as pool:
        recs = pool.map(_detect, range(N_KEYFRAMES), chunksize=8)
    res["detect_batch_s"] = time.perf_counter() - t0
    res["gated_pairs"] = int(sum(r["n_gated"] for r in recs))
    res["loops"] = int(sum(r["loop_id"] != -1 for r in recs))
    res["last"] = recs[-1]
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", default="")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    elif a.restatement:
        restatement(a.jobs)
    else:
        device()
