"""Per-phase times of the radix pass from the profiling build's in-kernel stamps (-DNDT_SORT_STAMPS):

    make -C xchu_slam_amd/csrc VARIANT=sortdbg VFLAGS=-DNDT_SORT_STAMPS
    NDT_HIP_LIB=libndt_hip_sortdbg.so python tools/sort_phases.py c2 [bench.py arguments]

Runs the bench workload in this process (warm-up included), then prints for every instantiation and pass the mean
time from a tile's start to the end of each phase, for the first, the middle and the last tile.  Every stamp follows a
workgroup barrier, so the phases do not overlap as they do in the product build: the table attributes, it does not time.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from xchu_slam_amd import _lib  # noqa: E402

WORDS = 16
PHASES = ("loads", "rank", "agg", "lookback", "scatter")


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "c2"
    rc = bench.main(["--workload", wl, "--no-cpu-baseline"] + (sys.argv[2:] or ["--steps", "20", "--warmup", "2"]))
    lib = C.CDLL(_lib.LIB_PATH)
    buf = (C.c_ulonglong * (3 * 4 * 3 * WORDS))()
    lib.ndt_dbg_read_sort.argtypes = [C.POINTER(C.c_ulonglong), C.c_size_t, C.c_int]
    err = lib.ndt_dbg_read_sort(buf, len(buf), 0)
    if err:
        print(f"ndt_dbg_read_sort: hip error {err}")
        return 1
    print(f"# {wl}: us from the tile's start to the end of each phase (mean over launches); start = the tile's start after the first tile's, last launch")
    print(f"{'keys/tile':>9} {'pass':>4} {'tile':>6} {'tiles':>6} {'launches':>8} " + " ".join(f"{p:>9}" for p in PHASES) + f" {'start':>8}")
    for vi, keys in enumerate((1024, 4096, 6144)):
        for ps in range(4):
            t0_first = buf[((vi * 4 + ps) * 3) * WORDS + 8]
            for ci, cname in enumerate(("first", "middle", "last")):
                row = buf[((vi * 4 + ps) * 3 + ci) * WORDS:((vi * 4 + ps) * 3 + ci + 1) * WORDS]
                if not row[0]:
                    continue
                us = [row[1 + k] / row[0] / 100.0 for k in range(5)]
                start = (int(row[8]) - int(t0_first)) / 100.0 if t0_first else 0.0
                print(f"{keys:>9} {ps:>4} {cname:>6} {row[6]:>6} {row[0]:>8} " + " ".join(f"{u:9.2f}" for u in us) + f" {start:8.2f}")
    return rc or 0


if __name__ == "__main__":
    sys.exit(main())
