#!/usr/bin/env python3
"""Times of the Scan Context path (profiles/scancontext.md): k_sc_make on a 120 k-point scan, one ndt_sc_detect against
1541 stored keyframes (the reference run's keyframe count), one ndt_sc_detect_batch over all 1541.

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python tools/sc_profile.py   # the workload, traced
    python tools/sc_profile.py --summarise DIR/run_kernel_trace.csv                             # kernel times
    python tools/sc_profile.py --restatement                                                    # tests/sc_restate.py, no GPU

The workload runs its three cases in a fixed order (WARMUP + REPEATS adds of the big scan, the 1541 keyframe adds,
WARMUP + REPEATS single detections, 1 + BATCH_REPEATS batches) and prints the host wall time of each call (launches,
synchronise, record copy) as one JSON line; --summarise picks each case's dispatches out of the trace by that order and
prints the median, minimum and maximum kernel time of the timed ones.  --restatement times the numpy restatement on the
same inputs (Python on the host, for scale only).

The 1541 keyframes are seeded random clouds (3000 points, uniform over a 60 m disc, heights -1.5..8 m): every bin is
populated, so no column is skipped in phase 2 — the costliest case for k_sc_detect.
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


def keyframe(i, n=3000):
    rng = np.random.default_rng(40_000 + i)
    r = 60.0 * np.sqrt(rng.uniform(0, 1, n))
    a = rng.uniform(0, 2 * np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.5, 8.0, n)], 1).astype(np.float32)


def big_scan():
    from xchu_slam_amd import synth
    world = synth.make_world(3, half=110.0)
    return synth.sensor_scan(world, synth.pose_matrix(0.0, 0.0, 1.73, 0.0, 0.0, 0.3), N_SCAN, 11, max_range=80.0)


def med(v):
    return float(statistics.median(v))


def synced_call(sc, f):
    """Host wall time (ms) of f() followed by a synchronise of the context."""
    t0 = time.perf_counter()
    out = f()
    assert sc._lib.ndt_synchronize(sc.ctx) == 0
    return (time.perf_counter() - t0) * 1e3, out


def device():
    import xchu_slam_amd as xa
    from xchu_slam_amd import synth
    res = {}
    scan = synth.to_xyz4(big_scan())
    with xa.SCManager(tree_making_period=1) as sc:
        lib, ctx = sc._lib, sc.ctx
        d = C.c_void_p()
        assert lib.ndt_device_alloc(ctx, scan.nbytes, C.byref(d)) == 0
        assert lib.ndt_memcpy_h2d(ctx, d, scan.ctypes.data_as(C.c_void_p), scan.nbytes) == 0
        wall = [synced_call(sc, lambda: sc.makeAndSaveScancontextAndKeysDevice(d.value, len(scan)))[0]
                for _ in range(WARMUP + REPEATS)][WARMUP:]
        lib.ndt_device_free(ctx, d)
        res["make_120k"] = {"ms_wall_call": med(wall), "points": len(scan), "bytes_read": scan.nbytes}
    with xa.SCManager(tree_making_period=1) as sc:
        for i in range(N_KEYFRAMES):
            sc.makeAndSaveScancontextAndKeys(keyframe(i))
        wall = [synced_call(sc, sc.detectLoopClosureID)[0] for _ in range(WARMUP + REPEATS)][WARMUP:]
        rec = sc.last_result()
        res["detect_one"] = {"ms_wall_call": med(wall), "stored": len(sc), "n_search": len(sc) - 30, "cand_idx": rec["cand_idx"],
                             "min_dist": rec["min_dist"]}
        query = np.arange(len(sc))
        sched = xa.scancontext.search_schedule(len(sc), 1, 30)
        runs = [synced_call(sc, lambda: sc.detect_batch(query, sched)) for _ in range(1 + BATCH_REPEATS)][1:]
        res["detect_batch"] = {"ms_wall_call": med([w for w, _ in runs]), "queries": len(query),
                               "searched": int(sum(1 for v in sched if v > 0)), "last_cand_idx": runs[-1][1][-1]["cand_idx"]}
    print(json.dumps(res))


def summarise(path):
    """Kernel times out of a rocprofv3 kernel trace of device(), by the order of the dispatches."""
    by = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("ndt::", "")
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    big = WARMUP + REPEATS
    assert len(by["k_sc_make"]) == big + N_KEYFRAMES and len(by["k_sc_finalize"]) == big + N_KEYFRAMES, {k: len(v) for k, v in by.items()}
    assert len(by["k_sc_detect"]) == big + 1 + BATCH_REPEATS, len(by["k_sc_detect"])
    cases = {"k_sc_make, 120k points": by["k_sc_make"][WARMUP:big], "k_sc_finalize": by["k_sc_finalize"][WARMUP:big],
             "k_sc_make, 3000 points": by["k_sc_make"][big:], "k_sc_detect, one query": by["k_sc_detect"][WARMUP:big],
             "k_sc_detect, batch": by["k_sc_detect"][big + 1:]}
    for name, v in cases.items():
        print(f"{name:28s} n {len(v):5d}  median {med(v):8.2f} us  min {min(v):8.2f}  max {max(v):8.2f}")


def restatement():
    import sc_restate as R
    res = {}
    scan = big_scan()
    t0 = time.perf_counter()
    R.make_scancontext(scan)
    res["make_120k_s"] = time.perf_counter() - t0
    descs = [R.make_scancontext(keyframe(i)) for i in range(N_KEYFRAMES)]
    rkeys = [R.ring_key(d) for d in descs]
    n = len(descs)
    t0 = time.perf_counter()
    rec = R.detect_one(descs, rkeys, n - 1, n - 30)
    res["detect_one_s"] = time.perf_counter() - t0
    res["detect_one_cand_idx"] = rec["cand_idx"]
    t0 = time.perf_counter()
    sched = R.search_schedule(n, 1, 30)
    recs = [R.detect_one(descs, rkeys, q, sched[q]) for q in range(n)]
    res["detect_batch_s"] = time.perf_counter() - t0
    res["last_cand_idx"] = recs[-1]["cand_idx"]
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", default="")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    elif a.restatement:
        restatement()
    else:
        device()
