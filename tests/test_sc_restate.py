"""Known answers of the Scan Context restatement (tests/sc_restate.py, the oracle of tests/test_gpu_scancontext.py) and
the layout of the two new C-ABI structs.  No GPU.

A point with x == 0, y > 0 lands in sector 15, not 16: atanf(inf) is the f32 above pi/2 (1.5707964f) and (180/M_PI)
times it is 90.0000025 in f64, but xy2theta returns a float (Scancontext.cpp:23), one f32 ulp at 90 is 7.6e-6, so the
angle comes back as exactly 90.0f and ceil(90 / 360 * 60) = 15.  The test pins both halves: the f64 product above 90, and
sector 15 after the narrowing; the first f32 above 90 degrees is in 16.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import sc_restate as R
from conftest import ROOT


def bin_of(x, y, z=0.0):
    """(ring, sector) 1-based of the one non-empty bin of a single-point scan with z + 2 != 0."""
    d = R.make_scancontext(np.array([[x, y, z]], np.float32))
    nz = np.argwhere(d != 0)
    assert len(nz) == 1, nz
    return int(nz[0][0]) + 1, int(nz[0][1]) + 1


def random_desc(seed, n=3000, spread=70.0):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-spread, spread, (n, 3)).astype(np.float32)
    pts[:, 2] = rng.uniform(-1.5, 8.0, n)
    return R.make_scancontext(pts)


# ---------------------------------------------------------------------------------------------- makeScancontext
def test_axis_points():
    assert bin_of(5.0, 0.0) == (2, 1)        # y == 0, x > 0: theta 0, ceil(0) = 0 clamps to sector 1
    assert bin_of(-5.0, 0.0) == (2, 30)      # y == 0, x < 0: theta exactly 180
    assert bin_of(0.0, -5.0) == (2, 45)      # 360 - 90
    # x == 0, y > 0 (see the module docstring)
    a = np.float32(np.arctan(np.float64(np.inf)))
    assert float(a) > math.pi / 2 and R.K_DEG * float(a) > 90.0
    assert np.float32(R.K_DEG * float(a)) == np.float32(90.0)
    assert bin_of(0.0, 5.0) == (2, 15)
    # the first direction past it: theta = the f32 after 90
    y = np.float32(5.0)
    x = -np.float32(2e-6)
    _, sector, _, _ = R._bins(np.array([x]), np.array([y]))
    assert sector[0] == 16 and bin_of(float(x), float(y)) == (2, 16)


def test_range_edges():
    assert bin_of(80.0, 0.0) == (20, 1)      # r == 80 is kept, ring 20
    assert not R.make_scancontext(np.array([[np.nextafter(np.float32(80.0), np.float32(100.0)), 0.0, 0.0]], np.float32)).any()
    assert bin_of(0.0, 0.0) == (1, 1)        # 0/0: NaN angle converts to INT_MIN on x86, clamped to 1; ring ceil(0) -> 1
    assert bin_of(4.0, 0.0) == (1, 1)        # r == 4 is the outer edge of ring 1 (ceil)
    assert bin_of(np.nextafter(np.float32(4.0), np.float32(5.0)), 0.0) == (2, 1)
    assert bin_of(3.0, 4.0) == (2, 9)        # r == 5, theta 53.13 deg


def test_bin_keeps_the_maximum_height_as_f32():
    pts = np.array([[10.0, 1.0, 0.5], [10.1, 1.0, 3.25], [10.2, 1.0, -1.0], [10.0, 0.9, 0.1]], np.float32)
    d = R.make_scancontext(pts)
    assert np.count_nonzero(d) == 1 and d[2, 0] == 5.25
    z = np.float32(0.1)
    d = R.make_scancontext(np.array([[10.0, 1.0, z]], np.float32))
    assert d[2, 0] == float(np.float32(np.float64(z) + 2.0))   # an f32 value held in a double


def test_nothing_above_no_point_gives_the_zero_descriptor():
    pts = np.array([[10.0, 1.0, -1002.0], [20.0, -3.0, -1500.0], [1.0, 1.0, -2000.0]], np.float32)
    assert np.float32(np.float64(pts[0, 2]) + 2.0) == np.float32(-1000.0)
    assert not R.make_scancontext(pts).any()
    assert not R.make_scancontext(np.zeros((0, 3), np.float32)).any()


def test_eigen_order():
    """Four lane sums, then (L0 + L2) + (L1 + L3): distinguishable from the plain left-to-right sum."""
    v = np.array([1e16, 1.0, -1e16, 1.0] + [0.0] * 16)
    assert R.esum(v) == 2.0                      # (1e16 + -1e16) + (1 + 1)
    assert ((v[0] + v[1]) + v[2]) + v[3] == 1.0  # left to right, the first 1 is lost
    w = np.array([0.1, 0.2, 0.3, 0.4] * 15)
    lanes = [0.0] * 4
    for i, x in enumerate(w):
        lanes[i % 4] = x if i < 4 else lanes[i % 4] + x
    assert R.esum(w) == (lanes[0] + lanes[2]) + (lanes[1] + lanes[3])
    assert R.esum(np.stack([w, v.repeat(3)])).shape == (2,)


def test_keys():
    d = random_desc(1)
    rk, sk = R.ring_key(d), R.sector_key(d)
    assert rk.dtype == np.float32 and sk.dtype == np.float64 and rk.shape == (20,) and sk.shape == (60,)
    assert np.allclose(rk, d.mean(1), rtol=1e-6) and np.allclose(sk, d.mean(0), rtol=1e-12)


# ---------------------------------------------------------------------------------------------- distances
def test_self_distance():
    d = random_desc(2)
    dist, shift = R.distance(d, d)
    # every counted column's cosine is dot / (sqrt(dot) * sqrt(dot)): within 2 ulp of 1, and so is their mean
    assert shift == 0 and abs(dist) <= 4 * 2.0 ** -52


@pytest.mark.parametrize("k", [1, 29, 59])
def test_rolled_copy_gives_the_complementary_shift(k):
    d = random_desc(3)
    rolled = np.roll(d, k, axis=1)
    dist, shift = R.distance(d, rolled)
    assert shift == 60 - k and abs(dist) <= 4 * 2.0 ** -52
    dist, shift = R.distance(rolled, d)
    assert shift == k and abs(dist) <= 4 * 2.0 ** -52


def test_zero_descriptor_is_nan_and_never_selected():
    d, zero = random_desc(4), np.zeros((20, 60))
    assert math.isnan(R.dist_direct(zero, d)) and math.isnan(R.dist_direct(d, zero))
    # no shift's NaN wins the reference's `<`: distanceBtnScanContext hands back its initial minimum and shift 0
    assert R.distance(d, zero) == (R.BIG, 0)
    m = R.SCManager(num_exclude_recent=1, num_candidates=3, tree_making_period=1)
    m.saveScancontextAndKeys(zero)
    m.saveScancontextAndKeys(random_desc(5))
    m.saveScancontextAndKeys(d)
    m.saveScancontextAndKeys(d)
    loop_id, _ = m.detectLoopClosureID()   # searchable: the zero descriptor, a stranger and d's copy
    assert sorted(m.last["cand_idx"]) == [0, 1, 2] and m.last["nn_idx"] == 2 and loop_id == 2
    assert m.last["cand_dist"][m.last["cand_idx"].index(0)] == R.BIG


def test_empty_columns_are_not_counted():
    d = random_desc(6)
    e = d.copy()
    e[:, 10:25] = 0.0
    assert abs(R.dist_direct(d, e)) <= 4 * 2.0 ** -52      # the 45 columns left are equal


def test_search_space_wraps_and_first_minimum_wins():
    assert R.search_radius(0.1) == 3 and R.search_radius(1.0) == 30 and R.search_radius(0.0) == 0
    d = random_desc(7)
    assert R.distance(d, np.roll(d, 2, axis=1), search_ratio=0.0) == R.distance(d, np.roll(d, 2, axis=1), search_ratio=1.0)


def test_yaw_diff_goes_through_float():
    assert R.deg2rad_f32(0.0) == 0 and R.deg2rad_f32(6.0 * 30) == np.float32(math.pi)
    assert R.deg2rad_f32(6.0 * 7).dtype == np.float32


# ---------------------------------------------------------------------------------------------- detection
def test_ring_distance_is_f32_in_groups_of_four():
    rng = np.random.default_rng(8)
    keys = rng.uniform(0, 5, (50, 20)).astype(np.float32)
    d2 = R.ring_dist2(keys[0], keys)
    assert d2.dtype == np.float32 and d2[0] == 0
    assert np.allclose(d2, ((keys - keys[0]).astype(np.float64) ** 2).sum(1), rtol=1e-5)


def test_early_return_and_stale_searchable_set():
    m = R.SCManager()
    for i in range(30):
        m.saveScancontextAndKeys(random_desc(100 + i, n=300))
        assert m.detectLoopClosureID() == (-1, 0.0) and m.counter == 0 and m.last["cand_idx"] == []
    sizes = []
    for i in range(30, 95):
        m.saveScancontextAndKeys(random_desc(100 + i, n=300))
        m.detectLoopClosureID()
        sizes.append(m.searchable)
        assert max(m.last["cand_idx"]) < m.searchable and len(m.last["cand_idx"]) == min(3, m.searchable)
    # rebuilt at 31 descriptors (1 key), stale for the 29 detections after it, rebuilt at 61 (31 keys) and at 91 (61)
    assert sizes == [1] * 30 + [31] * 30 + [61] * 5
    assert R.search_schedule(95) == [0] * 30 + sizes
    assert R.search_schedule(40, tree_making_period=1) == [0] * 30 + list(range(1, 11))


def test_package_schedule_matches():
    from xchu_slam_amd.scancontext import search_schedule
    for n, p, e in [(95, 30, 30), (70, 1, 30), (20, 7, 3), (0, 30, 30)]:
        assert search_schedule(n, p, e) == R.search_schedule(n, p, e)


def test_lower_index_wins_equal_ring_distances():
    d = [random_desc(200 + i, n=300) for i in range(4)]
    descs = [d[0], d[1], d[0], d[2], d[3], d[0]]     # 0 and 2 are the same place; 5 is the query
    rk = [R.ring_key(x) for x in descs]
    rec = R.detect_one(descs, rk, 5, 5, num_candidates=1)
    assert rec["cand_idx"] == [0] and rec["tie"]
    rec = R.detect_one(descs, rk, 5, 5, num_candidates=2)
    assert rec["cand_idx"] == [0, 2] and rec["nn_idx"] == 0 and rec["tie"]   # equal distances: the first stays (strict <)


# ---------------------------------------------------------------------------------------------- C-ABI layout
def test_sc_struct_layouts(tmp_path):
    """ctypes.sizeof and every field offset of ndt_sc_params / ndt_sc_result against the compiled header."""
    from xchu_slam_amd import _lib
    structs = {"ndt_sc_params": _lib.ScParams, "ndt_sc_result": _lib.ScResult}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "ndt_hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        src.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            src.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert ctypes.sizeof(_lib.ScResult) == 288 and ctypes.sizeof(_lib.ScParams) == 32


def test_sc_defaults_and_null_arguments():
    from xchu_slam_amd import _lib
    lib = _lib.load()
    p = _lib.ScParams()
    assert lib.ndt_sc_default_params(ctypes.byref(p)) == 0
    assert (p.dist_thres, p.num_exclude_recent, p.num_candidates, p.tree_making_period, p.search_ratio) == (0.2, 30, 3, 30, 0.1)
    assert lib.ndt_sc_default_params(None) == _lib.NDT_EINVAL
    assert lib.ndt_sc_create(None, None, None) == _lib.NDT_EINVAL
    assert lib.ndt_sc_size(None) == -1
    assert lib.ndt_sc_detect(None, None) == _lib.NDT_EINVAL
    lib.ndt_sc_destroy(None)
