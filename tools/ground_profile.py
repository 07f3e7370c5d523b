"""Ground detection on a KITTI-sized filtered scan: the whole call's host wall time, the restatement's time beside it,
and (from a rocprofv3 kernel trace of the same workload) the kernel times of the normals, the sampler, the scoring per
batch and the finish.  Writes profiles/ground.md.

    python tools/ground_profile.py --json OUT.json                       # wall times and the restatement (one process)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ground_profile.py --no-cpu --detects 30
    python tools/ground_profile.py --render OUT.json --kernel-stats DIR  # no GPU: writes the file from the two runs

Every number is printed; profiles/ground.md records one session's.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("k_ground_clip_flags", "k_ground_normals", "k_ground_sample", "k_ground_score", "k_ground_finish", "k_ground_origin",
           "k_ground_unmarked", "k_transform_mat", "k_compact4", "k_scan_onepass", "k_radix_onesweep", "k_keys", "k_minmax",
           "k_fit_gather", "k_fit_tables", "k_fit_block_flags", "k_fit_block_clear", "k_seg_scan")


def workload():
    import ground_scene as gs
    return gs.scene(0, radius=45.0)  # about the size of a KITTI scan after filter_node's 0.5 m front end


def med(f, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def measure(a):
    import xchu_slam_amd as xa
    cloud = workload()
    out = {"points": int(len(cloud)), "detects": a.detects}
    cf = xa.CloudFilter(cloud_leaf=0.0)
    t0 = time.perf_counter()
    r = cf.detect_plane(cloud)
    out["cold_ms"] = (time.perf_counter() - t0) * 1e3
    for _ in range(3):
        cf.detect_plane(cloud)
    out["detect_ms"] = med(lambda: cf.detect_plane(cloud), a.detects)
    out.update(batch=cf.batch, n_clipped=r.n_clipped, n_normal=r.n_normal, n_inliers=r.n_inliers, iterations=r.iterations,
               found=r.found, coeffs=[float(v) for v in r.coeffs] if r.found else None)

    def with_clouds(leaf):
        cf.set_params(cloud_leaf=leaf)

        def run():
            res = cf.detect_plane(cloud)
            res.normal_ground(), res.ground(), res.no_ground()
        run()
        return med(run, max(3, a.detects // 3))

    out["detect_clouds_raw_ms"] = with_clouds(0.0)
    out["detect_clouds_leaf_ms"] = with_clouds(0.2)
    cf.set_params(cloud_leaf=0.0, use_normal_filtering=0)
    cf.detect_plane(cloud)
    out["detect_no_normals_ms"] = med(lambda: cf.detect_plane(cloud), a.detects)
    cf.close()
    if not a.no_cpu:
        import ground_restate as gr
        t1 = time.perf_counter()
        ref = gr.detect(cloud)
        out["restatement_ms"] = (time.perf_counter() - t1) * 1e3
        t1 = time.perf_counter()
        clipped = cloud[gr.clip_mask(cloud)]
        gr.normals(clipped)
        out["restatement_normals_ms"] = (time.perf_counter() - t1) * 1e3
        out["restatement_same"] = bool(ref["found"] == r.found and ref["iterations"] == r.iterations and ref["n_inliers"] == r.n_inliers)
    for k, v in out.items():
        print(f"{k}: {v}")
    return out


def kernel_rows(stats_dir):
    """name -> (launches, median us) from a rocprofv3 kernel trace under stats_dir: its rocpd database (the `kernels`
    view) or its kernel_trace.csv.  The sampler and the scoring kernel are launched twice per detect (one chain); on this
    workload the first launch of a pair does the work and the second finds the loop ended, so the two are listed apart."""
    durs = {}
    for path in glob.glob(os.path.join(stats_dir, "**", "*_results.db"), recursive=True):
        import sqlite3
        db = sqlite3.connect(path)
        for name, dur in db.execute("select name, duration from kernels order by start"):
            durs.setdefault(name, []).append(dur / 1e3)
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            recs = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        for r in recs:
            durs.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = {}
    for k in KERNELS:
        d = [v for name, vs in durs.items() if k in name for v in vs] if k not in ("k_ground_sample", "k_ground_score") else \
            next((vs for name, vs in durs.items() if k in name), [])
        if not d:
            continue
        if k in ("k_ground_sample", "k_ground_score"):
            rows[k + " (first of a chain: a batch of 32)"] = (len(d[0::2]), statistics.median(d[0::2]))
            rows[k + " (second: the loop has ended)"] = (len(d[1::2]), statistics.median(d[1::2]))
        else:
            rows[k] = (len(d), statistics.median(d))
    return rows


def render(m, rows, path):
    lines = ["# Ground detection: first measured times", "",
             f"Workload: `tests/ground_scene.scene(0, radius=45)`, {m['points']} points (a KITTI-sized scan after the 0.5 m front end); "
             f"{m['n_clipped']} after the height clip, {m['n_normal']} after the normal filter, {m['n_inliers']} inliers, "
             f"{m['iterations']} RANSAC iterations.  B = {m['batch']} hypotheses per scoring launch (`kGroundBatch`); one chain of launches "
             "(2 x (sample, score) + finish) ends the fit.  Produced by `tools/ground_profile.py`; MI355X, one process.", "",
             "## Whole call (host wall time, median)", "",
             "| call | ms |", "|---|---|",
             f"| first `ndt_ground_detect` of the context (allocations, generator table upload) | {m['cold_ms']:.3f} |",
             f"| `ndt_ground_detect`, host cloud in, result record out (median of {m['detects']}) | {m['detect_ms']:.3f} |",
             f"| the same with `use_normal_filtering = 0` (no neighbour index, no normals) | {m['detect_no_normals_ms']:.3f} |",
             f"| detect + the three clouds, raw | {m['detect_clouds_raw_ms']:.3f} |",
             f"| detect + the three clouds through the 0.2 m VoxelGrid | {m['detect_clouds_leaf_ms']:.3f} |"]
    if "restatement_ms" in m:
        lines += [f"| numpy restatement of the detect, 16 cores for the tree queries | {m['restatement_ms']:.0f} |",
                  f"| of which clip + neighbours + normals | {m['restatement_normals_ms']:.0f} |", "",
                  f"Device and restatement agree on found / iterations / inliers: {m['restatement_same']}."]
    lines += ["", "## Kernels (rocprofv3 --kernel-trace --stats over the same workload)", ""]
    if rows:
        lines += ["| kernel | launches | median us |", "|---|---|---|"]
        for k, (n, us) in rows.items():
            lines.append(f"| `{k}` | {n} | {us:.2f} |")
        lines += ["", "Launch counts are those of the traced run (its warm-up and cloud requests included).  The sort, scan and index "
                  "kernels are the clipped cloud's neighbour index and the compactions.  Under the tracer no launch measures below "
                  "about 4 us and launches do not overlap, so the rows add up to more than the untraced call above.", "",
                  "## Reading", "",
                  f"* B = {m['batch']}: scoring a batch of {m['batch']} planes over the {m['n_normal']} points is one launch; this scan's fit "
                  f"took {m['iterations']} iterations, inside the first batch, and every later launch of the chain returned at its first load.",
                  "* The sampler is one lane walking dependent loads (generator words, the hash of touched positions, three points per "
                  "check): it makes all of a batch's samples ahead of the scoring, of which a typical fit uses a handful.",
                  "* `k_ground_normals` (neighbour walk, f64 moments, the 3x3 eigen solve by the team's first lane) and the neighbour "
                  "index in front of it are the larger half of the call: without the normal filter the call takes "
                  f"{m['detect_no_normals_ms']:.3f} ms instead of {m['detect_ms']:.3f} ms."]
    else:
        lines.append("No kernel trace was available for this session.")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detects", type=int, default=30)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", help="write the measurements here")
    ap.add_argument("--render", help="measurements written by --json: write the profile from them, no GPU")
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground.md"))
    a = ap.parse_args()
    if a.render:
        with open(a.render) as f:
            m = json.load(f)
        render(m, kernel_rows(a.kernel_stats) if a.kernel_stats else {}, a.out)
        return 0
    m = measure(a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(m, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
