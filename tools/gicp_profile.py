"""GICP on the loop-sized pair of profiles/icp_loop_pair.md (15 k points against 163 k): host wall times of the
covariances, a cold and a warm align, launches and host round trips, ICP beside it, and the CPU restatement.

    python tools/gicp_profile.py                 # the table (one process)
    python tools/gicp_profile.py --ab            # round A/B: one child process per NDT_GICP_GRAPH x NDT_GICP_ROUND, interleaved, 3 repeats
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gicp_profile.py --aligns 10 --no-cpu    # kernel times

Every number is printed; profiles/gicp.md records one session's.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def loop_pair():
    from xchu_slam_amd import synth
    import icp_restate as R
    world = synth.make_world(11, half=80.0)
    pair = synth.make_pair(world, 5.0, 15000, seed=23, max_range=60.0)
    src = R.transform_f32(pair.guess.astype(np.float32), pair.source)
    return pair.target.astype(np.float32), src


def med(f, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aligns", type=int, default=15)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.ab:
        for rep in range(3):
            for graph, blocks in [(g, b) for g in (1, 0) for b in (1, 2, 4, 8)]:
                env = dict(os.environ, NDT_GICP_ROUND=str(blocks), NDT_GICP_GRAPH=str(graph))
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--aligns", str(a.aligns)], env=env,
                                     capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    print(out.stdout + out.stderr)
                    return out.returncode
                print(f"repeat {rep + 1} NDT_GICP_GRAPH={graph} NDT_GICP_ROUND={blocks}: {out.stdout.strip()}", flush=True)
        return 0

    import xchu_slam_amd as xa
    tgt, src = loop_pair()
    g = xa.GeneralizedIterativeClosestPoint()
    g.setResolution(1.0)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    t0 = time.perf_counter()
    g.align(want_output=False)
    cold = (time.perf_counter() - t0) * 1e3
    for _ in range(3):
        g.align(want_output=False)
    warm = med(lambda: g.align(want_output=False), a.aligns)
    r, st = g.result(), g.run_stats()
    if a.child:
        print(f"warm align {warm:.3f} ms, launches {st['launches']}, round trips {st['round_trips']}")
        return 0
    print(f"pair: target {len(tgt)} points, source {len(src)} points")
    print(f"GICP: {r['nr_iterations']} outer iterations, state {r['state']}, {r['n_evals']} evaluations, pairs {r['n_pairs']}, f {r['f']:.9g}")
    print(f"launches per align {st['launches']}, host round trips {st['round_trips']}")
    print(f"cold align (index + covariances of both clouds + align): {cold:.3f} ms")
    print(f"warm align (covariances kept): {warm:.3f} ms (median of {a.aligns})")

    def fresh_cov():
        g.setInputTarget(tgt)
        g.setInputSource(src)
        t1 = time.perf_counter()
        g._lib.ndt_synchronize(g.ctx)
        g.align(want_output=False)
        return (time.perf_counter() - t1) * 1e3

    print(f"align after setInputTarget + setInputSource (both covariances recomputed): {statistics.median([fresh_cov() for _ in range(5)]):.3f} ms")
    t_eval = med(lambda: g.evaluate(np.zeros(6)), 20)
    print(f"one evaluate() call (upload, one k_gicp_eval launch, read-back): {t_eval:.3f} ms")
    icp = xa.IterativeClosestPoint(registration=g.registration)
    icp.setMaxCorrespondenceDistance(150)
    icp.setMaximumIterations(100)
    icp.setTransformationEpsilon(1e-6)
    icp.setEuclideanFitnessEpsilon(1e-6)
    for _ in range(3):
        icp.align(want_output=False)
    print(f"ICP (pgo_node's settings) on the same pair: {med(lambda: icp.align(want_output=False), a.aligns):.3f} ms, "
          f"{icp.getFinalNumIteration()} iterations")
    if not a.no_cpu:
        import gicp_restate as G
        import icp_restate as R
        t1 = time.perf_counter()
        T = R.Target(tgt)
        cov_t = G.covariances(T.pts)[0]
        cov_s = G.covariances(src)[0]
        t2 = time.perf_counter()
        ref = G.gicp(src, tgt, tgt=T, cov_tgt=cov_t, cov_src=cov_s)
        t3 = time.perf_counter()
        print(f"restatement: tree + covariances {(t2 - t1) * 1e3:.0f} ms, align {(t3 - t2) * 1e3:.0f} ms, {ref['iterations']} iterations, "
              f"{ref['evals']} evaluations; |final - device final| max {float(np.max(np.abs(ref['final'] - r['final_tf']))):.3g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
