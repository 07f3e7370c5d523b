"""tests/isc_restate.py (the Intensity Scan Context oracle, parity unpinned) against cases worked out by hand, and the
condition that the loop route of tests/isc_scene.py exercises detection at all.  No GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import isc_restate as R
import isc_scene
from conftest import ROOT

YAWS = [0.0, 48.0, -45.0]


def column_desc(rings, sectors, col, values):
    d = np.zeros((rings, sectors), np.uint8)
    d[:, col] = values
    return d


# ---------------------------------------------------------------------------------------------- the two measures
def test_equals_true_quirk():
    """`at<uchar>() == true`: a byte matches as 1 or as 0, never as "non-zero"."""
    ones, twos, zeros = (np.full((3, 20), v, np.uint8) for v in (1, 2, 0))
    for lit in (False, True):
        assert R.calculate_geometry_dis(ones, ones, lit) == (1.0, 0)
        assert R.calculate_geometry_dis(twos, twos, lit) == (0.0, 0)      # identical descriptors, no match at all
        assert R.calculate_geometry_dis(zeros, zeros, lit) == (1.0, 0)
        assert R.calculate_geometry_dis(ones, twos, lit) == (0.0, 0)
        assert R.calculate_geometry_dis(ones, zeros, lit) == (0.0, 0)
    mixed = np.array([[0, 1, 2, 200] * 5], np.uint8)                      # 1 x 20: five each of 0, 1, 2, 200
    assert R.calculate_geometry_dis(mixed, mixed) == (10 / 20, 0)         # the zeros and the ones only
    assert R.geometry_counts(mixed, mixed).tolist() == [10, 0, 0, 0] * 5


def test_first_maximum_among_equal_shifts():
    base = np.zeros((2, 20), np.uint8)
    base[:, ::5] = 1                                                      # period 5: shifts 0, 5, 10, 15 are equal
    counts = R.geometry_counts(base, base)
    assert counts[0] == counts[5] == counts[10] == counts[15] == 40 and counts.max() == 40
    assert R.calculate_geometry_dis(base, base) == (1.0, 0)
    rolled = np.roll(base, 3, axis=1)                                     # desc2(q, p + 3) = desc1(q, p)
    assert R.calculate_geometry_dis(base, rolled) == (1.0, 3)
    assert R.calculate_geometry_dis(base, rolled, literal=True) == (1.0, 3)
    assert R.first_max([0, 0, 0]) == (0, 0) and R.first_max([2, 5, 5, 1]) == (5, 1)


def test_vectorised_equals_literal():
    rng = np.random.default_rng(3)
    for _ in range(4):
        a = rng.choice(np.array([0, 0, 1, 1, 2, 90, 255], np.uint8), (4, 20))
        b = rng.choice(np.array([0, 0, 1, 1, 2, 90, 255], np.uint8), (4, 20))
        assert R.geometry_counts(a, b).tolist() == R.geometry_counts_literal(a, b)
        for angle in (0, 7, 19):
            assert R.intensity_sads(a, b, angle) == R.intensity_sads(a, b, angle, literal=True)


def test_intensity_window_and_wrap():
    """One non-zero column of bytes (7, 100, 255): against a copy rolled by k columns the SAD is 0 at shift k and
    2 * 362 at every other shift."""
    rings, sectors, vals = 3, 60, [7, 100, 255]
    d1 = column_desc(rings, sectors, 4, vals)
    full = 2 * sum(vals) / (sectors * rings * 255)
    for angle, k, inside in [(59, 5, True),     # window 49 .. 68: shift 65 is column shift 5 (the reference leaves its row here)
                             (59, 49, True), (59, 8, True), (59, 9, False), (59, 48, False),
                             (0, 55, True),     # window -10 .. 9: shift -5
                             (0, 50, True), (0, 9, True), (0, 10, False), (0, 49, False),
                             (30, 20, True), (30, 39, True), (30, 40, False), (30, 19, False)]:
        d2 = np.roll(d1, k, axis=1)
        want = 1.0 if inside else 1 - full
        assert R.calculate_intensity_dis(d1, d2, angle) == want, (angle, k)
        assert R.calculate_intensity_dis(d1, d2, angle, literal=True) == want, (angle, k)
    assert len(R.intensity_sads(d1, d1, 0)) == 20
    # difference starts at 1.0: an SAD of the full scale gives 1 - 1.0
    assert R.calculate_intensity_dis(np.full((2, 20), 255, np.uint8), np.zeros((2, 20), np.uint8), 0) == 0.0


def test_is_loop_pair_order():
    a = np.zeros((2, 20), np.uint8)
    b = np.full((2, 20), 2, np.uint8)
    ok, geo, inten, angle = R.is_loop_pair(a, b)
    assert (ok, geo, inten, angle) == (False, 0.0, 0.0, 0)                # the intensity is not evaluated
    assert R.pair(a, b) == (0.0, 0, 1 - 2 / 255, False)                   # ndt_isc_pair evaluates it anyway
    assert R.is_loop_pair(a, a) == (True, 1.0, 1.0, 0)


# ---------------------------------------------------------------------------------------------- gate and detection
def test_gate_boundaries():
    origin, near = [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]
    assert not R.gate([0.0, 20.0], [origin, origin], 1, 0)                # delta exactly 20: strict >
    assert R.gate([0.0, math.nextafter(20.0, 30.0)], [origin, origin], 1, 0)
    assert 100.0 * 0.03 == 3.0
    assert not R.gate([0.0, 100.0], [near, origin], 1, 0)                 # pos exactly 0.03 * delta: strict <
    assert R.gate([0.0, 100.0], [[math.nextafter(3.0, 0.0), 0.0, 0.0], origin], 1, 0)
    assert not R.gate([0.0, 100.0], [origin, origin], 1, 1)               # the query itself: delta 0


def zigzag(descs):
    """Keyframe k at the origin (k even) or 30 m away (k odd): the even ones gate each other."""
    g = R.ISCGeneration(rings=2, sectors=20, max_dis=40.0)
    for k, d in enumerate(descs):
        g.add_descriptor(d, (30.0 * (k % 2), 0.0, 0.0))
    return g


def test_detection_rules():
    rng = np.random.default_rng(1)
    A = rng.integers(0, 2, (2, 20)).astype(np.uint8)
    other = np.full((2, 20), 9, np.uint8)
    # candidates 2 and 4 have the same sum: the strict > keeps the lower index; second = float(curr)
    g = zigzag([other, other, A, other, A, other, A])
    assert g.travel == [30.0 * k for k in range(7)]
    assert g.detectLoopClosureID() == (2, np.float32(6.0)) and isinstance(g.detectLoopClosureID()[1], np.float32)
    assert (g.last["best_id"], g.last["best_score"], g.last["n_gated"], g.last["n_loop_pairs"]) == (2, 2.0, 3, 2)
    # the winner is index 0: no loop, although index 2 passed too (with a lower sum)
    weaker = A.copy()
    weaker[0, :2] = 40                                                    # two cells off: geometry 38/40, intensity < 1
    g = zigzag([A, other, weaker, other, A])
    assert g.detectLoopClosureID() == (-1, np.float32(0.0))
    assert (g.last["best_id"], g.last["best_score"], g.last["n_loop_pairs"]) == (0, 2.0, 2)
    assert g.detect(2)["loop_id"] == -1 and g.detect(2)["best_id"] == 0 and g.detect(2)["n_loop_pairs"] == 1
    # no gated pair
    assert g.detect(1) == {"loop_id": -1, "curr_id": 1, "best_id": 0, "best_score": 0.0, "geo_score": 0.0, "inten_score": 0.0,
                           "angle": 0, "n_gated": 0, "n_geometry": 0, "n_loop_pairs": 0}


def test_position_is_narrowed_and_travel_accumulates():
    g = R.ISCGeneration(rings=2, sectors=20)
    z = np.zeros((2, 20), np.uint8)
    g.add_descriptor(z, (0.1, 0.0, 0.0))
    g.add_descriptor(z, (0.1, 3.0, 4.0))
    g.add_descriptor(z, (0.1, 3.0, 4.0))
    assert g.pos[0][0] == float(np.float32(0.1)) != 0.1
    assert g.travel == [0.0, 5.0, 5.0]


# ---------------------------------------------------------------------------------------------- binning edges
def one_point(x, y, z=0.0, w=0.5, **kw):
    d = R.calculate_isc(np.array([[x, y, z, w]], np.float32), **kw)
    return [(int(r), int(s), int(d[r, s])) for r, s in zip(*np.nonzero(d))]


def test_binning_edges():
    step = 2 * math.pi / 60
    assert math.floor(math.pi / step) in (29, 30)
    assert one_point(5.0, 0.0) == [(7, math.floor(math.pi / step), 127)]          # atan2 = 0: angle = pi
    assert one_point(0.0, 5.0) == [(7, 45, 127)]                                  # (float)(pi/2) > pi/2
    assert one_point(0.0, -5.0) == [(7, 14, 127)]                                 # pi - (float)(pi/2) < pi/2
    assert one_point(-5.0, 0.0) == []                                             # y = +0: angle >= 2 pi, sector 60
    assert one_point(-5.0, -0.0) == []                                            # y = -0: angle < 0, sector -1 (deviation 1)
    assert R.bin_ids([-5.0], [0.0])[1][0] == 60 and R.bin_ids([-5.0], [-0.0])[1][0] == -1
    assert one_point(0.0, 0.0) == [(0, math.floor(math.pi / step), 127)]
    below = np.nextafter(np.float32(40.0), np.float32(0.0))
    assert one_point(below, 0.0)[0][0] == 59 and one_point(40.0, 0.0) == []       # distance >= max_dis is skipped
    assert one_point(3.0, 4.0, z=np.float32(-0.9)) != [] and one_point(3.0, 4.0, z=np.float32(30.0)) != []
    assert one_point(3.0, 4.0, z=np.nextafter(np.float32(-0.9), np.float32(-1.0))) == []
    assert one_point(3.0, 4.0, z=np.nextafter(np.float32(30.0), np.float32(31.0))) == []
    assert one_point(3.0, 4.0, z=float("nan")) == [] and one_point(float("inf"), 4.0) == []
    # the second shape: 20 rings x 90 sectors over 60 m
    assert one_point(0.0, 31.0, rings=20, sectors=90, max_dis=60.0) == [(10, 67, 127)]


def test_intensity_byte():
    w = np.array([0.0, 1.0, 0.5, 0.999, 1 / 255, -0.5, 1.5, float("nan"), float("inf"), -float("inf")], np.float32)
    assert R.intensity_byte(w).tolist() == [0, 255, 127, 254, 1, 0, 255, 0, 255, 0]
    cloud = np.array([[3, 4, 0, 0.2], [3, 4, 0, 0.7], [3, 4, 0, 0.4], [3.01, 4, 0, 1.5], [-7, 2, 0, -0.5], [-7, 2, 0, float("nan")]], np.float32)
    d = R.calculate_isc(cloud)
    assert d.max() == 255 and np.count_nonzero(d) == 1                           # the maximum, clamped; the others 0


def test_color_table():
    t = R.color_table()
    assert t.shape == (272, 3) and t.dtype == np.uint8
    assert t[0].tolist() == [0, 0, 255] and t[-1].tolist() == [255, 252, 252]
    assert t[1].tolist() == [0, 0, 255] and t[16].tolist() == [0, 255, 255] and t[255].tolist() == [255, 188, 188]
    from xchu_slam_amd.isc import color_projection
    assert np.array_equal(color_projection(), t)


# ---------------------------------------------------------------------------------------------- the C structs
def test_ctypes_mirrors_match_the_header(tmp_path):
    from xchu_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    structs = {"ndt_isc_params": _lib.IscParams, "ndt_isc_result": _lib.IscResult}
    for cname, py in structs.items():
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names += [first.split()[-1]] + [r.strip() for r in rest]
        assert names == [f for f, _ in py._fields_], cname
    assert [t for _, t in _lib.IscParams._fields_] == [ctypes.c_int] * 2 + [ctypes.c_double] * 5 + [ctypes.c_float] * 2
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "ndt_hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        src.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        src += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py) == 56, cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert _lib.ABI_VERSION == 6 and "#define NDT_HIP_ABI_VERSION 6" in hdr
    p = _lib.IscParams()
    assert _lib.load().ndt_isc_default_params(ctypes.byref(p)) == 0
    assert (p.rings, p.sectors, p.max_dis) == (R.RINGS, R.SECTORS, R.MAX_DIS)
    assert (p.skip_neighbour_distance, p.inflation_covariance, p.geometry_threshold, p.intensity_threshold) == (20.0, 0.03, 0.67, 0.91)
    assert (np.float32(p.z_min), np.float32(p.z_max)) == (R.Z_MIN, R.Z_MAX)


# ---------------------------------------------------------------------------------------------- the route
@pytest.mark.parametrize("yaw", YAWS)
def test_route_exercises_detection(yaw):
    """Keyframes 79 .. 101 each detect the place of q - 78 or q - 79 (23 loops), nothing earlier does; a yaw offset of
    +48 deg shows as column shift 8, -45 deg as 52 or 53 — there every gated pair's window passes the last column, where
    the reference's single subtraction leaves its row."""
    scans, poses = isc_scene.route_keyframes(yaw_offset=math.radians(yaw))
    assert len(scans) == 102 and all(s.shape == (3000, 4) for s in scans)
    w = np.concatenate([s[:, 3] for s in scans])
    assert w.min() >= np.float32(30) / np.float32(255) and w.max() <= np.float32(229) / np.float32(255)
    g = R.ISCGeneration()
    recs = []
    for s, p in zip(scans, poses):
        g.makeAndSavedec(s, (p[0], p[1], 0.0))
        g.detectLoopClosureID()
        recs.append(g.last)
    loops = [r for r in recs if r["loop_id"] != -1]
    assert [r["curr_id"] for r in loops] == list(range(79, 102))
    assert all(r["curr_id"] - r["loop_id"] in (78, 79) for r in loops)
    assert all(0.82 <= r["geo_score"] <= 0.87 and 0.911 <= r["inten_score"] <= 0.945 for r in loops)
    want = {0.0: {0}, 48.0: {8}, -45.0: {52, 53}}[yaw]
    assert {r["angle"] for r in loops} == want
    assert len(g.cache) == 94                                                     # gated pairs in all
    if yaw == -45.0:
        assert all(v[3] >= 52 for v in g.cache.values())
