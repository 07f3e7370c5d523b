#!/usr/bin/env python3
"""Times of the global map path (profiles/globalmap.md).

    python tools/globalmap_profile.py --map                       # global map: one launch vs a launch per keyframe vs the CPU
    python tools/globalmap_profile.py --loop                      # refine_loop with and without a store
    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python tools/globalmap_profile.py --map --no-cpu
    python tools/globalmap_profile.py --summarise DIR/.../run_kernel_trace.csv

--map: 1541 keyframes at evenly spaced poses of the KITTI-00 trajectory (tests/golden/kitti00_gt.npz, 3724 m: one every
2.4 m), each a seeded cloud of N_POINTS points within 60 m of the sensor (filter_node's range crop), all resident in one
KeyframeMap.  Three ways to the same leaf-0.5 map, the first two alternating in one process and compared bit for bit:
  (a) ndt_map_build: one k_map_stack launch + VoxelGrid;
  (b) the calls the library had before: ndt_transform_device per keyframe (reading the resident keyframe) into one
      buffer + ndt_voxel_downsample_device;
  (c) the CPU restatement's VoxelGrid of the stacked cloud (OpenMP, the box's 16 cores).
Times are host wall clock around calls that end synchronised.

--loop: xa.refine_loop on a loop-sized pair (the pair of profiles/icp_loop_pair.md cut into 51 target keyframes and one
source keyframe) from host keyframes and from a store, alternating.
"""
import argparse
import csv
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_KEYFRAMES, N_POINTS, WARMUP, REPEATS, LEAF = 1541, 14_000, 2, 10, 0.5


def pose6d(T):
    """(x, y, z, roll, pitch, yaw) of T = Trans * Rz(yaw) * Ry(pitch) * Rx(roll)."""
    return (float(T[0, 3]), float(T[1, 3]), float(T[2, 3]), math.atan2(T[2, 1], T[2, 2]), -math.asin(max(-1.0, min(1.0, T[2, 0]))),
            math.atan2(T[1, 0], T[0, 0]))


def trajectory():
    from xchu_slam_amd import synth
    tum = np.load(os.path.join(ROOT, "tests", "golden", "kitti00_gt.npz"))["tum"]
    sel = np.round(np.linspace(0, len(tum) - 1, N_KEYFRAMES)).astype(int)
    return [pose6d(T) for T in synth.kitti_poses(tum)[sel]]


def keyframe(i):
    rng = np.random.default_rng(70_000 + i)
    r = 60.0 * np.sqrt(rng.uniform(0.0003, 1.0, N_POINTS))   # 1 m .. 60 m, uniform over the disc
    a = rng.uniform(0, 2 * np.pi, N_POINTS)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.8, 8.0, N_POINTS), rng.uniform(0, 1, N_POINTS)], 1).astype(np.float32)


def stats(v):
    return {"median": float(statistics.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def run_map(cpu: bool):
    import xchu_slam_amd as xa
    from xchu_slam_amd import _lib
    poses = trajectory()
    res = {"keyframes": N_KEYFRAMES, "points_per_keyframe": N_POINTS, "leaf": LEAF}
    with xa.KeyframeMap() as m:
        lib, ctx, h = m._lib, m.ctx, m._handle
        m.reserve(N_KEYFRAMES * N_POINTS)
        for i in range(N_KEYFRAMES):
            m.add(keyframe(i))
        total = m.count(None)
        res["points"] = total
        T = np.concatenate([np.ascontiguousarray(xa.icp.get_transformation(*p).T).reshape(-1) for p in poses]).astype(np.float32)
        fp = C.POINTER(C.c_float)
        d_a, d_stack, d_b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for d in (d_a, d_stack, d_b):
            _lib.check(lib.ndt_device_alloc(ctx, total * 16, C.byref(d)), ctx)
        kf = [m.keyframe_device(i) for i in range(N_KEYFRAMES)]
        offs = np.concatenate([[0], np.cumsum([n for _, n in kf])])
        n_a, n_b = C.c_size_t(), C.c_size_t()

        def build_a():
            _lib.check(lib.ndt_map_build(h, None, T.ctypes.data_as(fp), N_KEYFRAMES, LEAF, d_a, total, C.byref(n_a)), ctx)

        def stack_a():
            _lib.check(lib.ndt_map_build(h, None, T.ctypes.data_as(fp), N_KEYFRAMES, 0.0, d_a, total, C.byref(n_a)), ctx)

        # (b)'s arguments ready-made, so that its loop costs what a C++ caller's would: one call per keyframe
        calls_b = [(C.cast(T.ctypes.data + 64 * k, fp), C.c_void_p(ptr), n, C.c_void_p(d_stack.value + 16 * int(offs[k])))
                   for k, (ptr, n) in enumerate(kf)]
        transform = lib.ndt_transform_device

        def stack_b():
            for Tk, src, n, dst in calls_b:
                if transform(ctx, Tk, src, n, dst) != 0:
                    raise RuntimeError("ndt_transform_device failed")

        def build_b():
            stack_b()
            _lib.check(lib.ndt_voxel_downsample_device(ctx, d_stack, total, LEAF, d_b, C.byref(n_b)), ctx)

        def timed(f):
            t0 = time.perf_counter()
            f()
            _lib.check(lib.ndt_synchronize(ctx), ctx)
            return (time.perf_counter() - t0) * 1e3

        times = {"a_map_build": [], "b_per_keyframe": [], "a_stack_only": [], "b_stack_only": []}
        for r in range(WARMUP + REPEATS):
            for name, f in (("a_map_build", build_a), ("b_per_keyframe", build_b), ("a_stack_only", stack_a), ("b_stack_only", stack_b)):
                ms = timed(f)
                if r >= WARMUP:
                    times[name].append(ms)
        res["ms"] = {k: stats(v) for k, v in times.items()}
        res["geometry"] = m.geometry()
        # the same map from both paths, bit for bit
        build_a()
        build_b()
        assert n_a.value == n_b.value
        out_a, out_b = np.empty((n_a.value, 4), np.float32), np.empty((n_b.value, 4), np.float32)
        _lib.check(lib.ndt_memcpy_d2h(ctx, out_a.ctypes.data_as(C.c_void_p), d_a, out_a.nbytes), ctx)
        _lib.check(lib.ndt_memcpy_d2h(ctx, out_b.ctypes.data_as(C.c_void_p), d_b, out_b.nbytes), ctx)
        assert np.array_equal(out_a.view(np.uint32), out_b.view(np.uint32))
        res["map_points"] = int(n_a.value)
        res["a_equals_b_bitwise"] = True
        # the Python entry point (pose conversion included)
        t0 = time.perf_counter()
        p, n = m.global_map(poses, LEAF, to_host=False)
        res["ms_global_map_python"] = (time.perf_counter() - t0) * 1e3
        assert n == n_a.value
        if cpu:
            import oracle_lib
            oracle_lib.build_oracle()
            stack = np.empty((total, 4), np.float32)
            stack_b()
            _lib.check(lib.ndt_synchronize(ctx), ctx)
            _lib.check(lib.ndt_memcpy_d2h(ctx, stack.ctypes.data_as(C.c_void_p), d_stack, stack.nbytes), ctx)
            cpu_ms = []
            for _ in range(2):
                t0 = time.perf_counter()
                ref = oracle_lib.voxel_downsample(stack, LEAF)
                cpu_ms.append((time.perf_counter() - t0) * 1e3)
            res["ms_c_cpu_voxelgrid_only"] = cpu_ms
            res["a_equals_cpu_bitwise"] = bool(ref.shape == out_a.shape and np.array_equal(ref.view(np.uint32), out_a.view(np.uint32)))
            res["omp_threads"] = os.environ.get("OMP_NUM_THREADS", "")
        for d in (d_a, d_stack, d_b):
            lib.ndt_device_free(ctx, d)
    print(json.dumps(res))


def loop_scene():
    from xchu_slam_amd import synth
    world = synth.make_world(11, half=80.0)
    pair = synth.make_pair(world, 5, 15000, 23, max_range=60.0)
    rng = np.random.default_rng(3)
    tgt = np.concatenate([pair.target, rng.uniform(0, 1, (len(pair.target), 1))], 1).astype(np.float32)
    src = np.concatenate([pair.source, rng.uniform(0, 1, (len(pair.source), 1))], 1).astype(np.float32)
    keyframes = [tgt[k::51] for k in range(51)] + [src]   # the target submap is root 25 +- 25; the source keyframe 51
    poses = [(0.0,) * 6] * 51 + [pose6d(pair.guess)]
    return keyframes, poses


def run_loop():
    import xchu_slam_amd as xa
    keyframes, poses = loop_scene()
    args = dict(loop_idx=25, curr_idx=51, search_num=25, leaf=LEAF)
    res = {"target_points": int(sum(len(k) for k in keyframes[:51])), "source_points": len(keyframes[51])}
    with xa.KeyframeMap() as m:
        for k in keyframes:
            m.add(k)
        times = {"host_keyframes": [], "store": []}
        outs = {}
        for r in range(3 + 10):
            for name, f in (("host_keyframes", lambda: xa.refine_loop(keyframes, poses, **args)),
                            ("store", lambda: xa.refine_loop(None, poses, store=m, **args))):
                t0 = time.perf_counter()
                outs[name] = f()
                if r >= 3:
                    times[name].append((time.perf_counter() - t0) * 1e3)
    a, b = outs["host_keyframes"], outs["store"]
    assert np.array_equal(a["transform"].view(np.uint32), b["transform"].view(np.uint32)) and a["score"] == b["score"]
    res.update(ms={k: stats(v) for k, v in times.items()}, iterations=a["iterations"], score=a["score"], accepted=a["accepted"],
               n_source=a["n_source"], n_target=a["n_target"], same_result=True)
    print(json.dumps(res))


def summarise(path):
    by = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("ndt::", "")
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print(f"{name:40s} n {len(v):7d}  median {statistics.median(v):10.2f} us  min {min(v):10.2f}  max {max(v):10.2f}  sum {sum(v) / 1e3:10.2f} ms")
    v = by.get("k_map_stack")
    if v:
        big = [t for t in v if t > 0.5 * max(v)]   # the whole-map launches (the loop / Python entry launches are not in --map)
        nbytes = 32.0 * N_KEYFRAMES * N_POINTS
        t = statistics.median(big)
        print(f"k_map_stack whole map: {len(big)} launches, median {t:.1f} us, {nbytes / 1e6:.1f} MB -> {nbytes / t / 1e6:.2f} TB/s "
              f"({100 * nbytes / t / 1e6 / 6.29:.0f} % of the 6.29 TB/s float4-copy rate)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", default="")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    if a.map:
        run_map(not a.no_cpu)
    if a.loop:
        run_loop()
