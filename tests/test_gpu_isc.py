"""Intensity Scan Context on the device (xa.ISCGeneration, xa.detect_loops_isc, xa.close_loops(loop_method=2)) against
tests/isc_restate.py.  Every comparison is exact: bytes, integers, and f64 scores as bits.

After the binning everything is integer arithmetic and quotients of integers.  The binning itself needs the device's and
numpy's f64 arctangent to round to the same f32; the points placed on an edge on purpose are exact by construction."""
import ctypes as C
import math

import numpy as np
import pytest

import isc_restate as R
import isc_scene
import sc_scene

pytestmark = pytest.mark.gpu

YAWS = [0.0, 48.0, -45.0]
RESULT_KEYS = ("loop_id", "curr_id", "best_id", "angle", "n_gated", "n_geometry", "n_loop_pairs")
SCORE_KEYS = ("best_score", "geo_score", "inten_score")


def f64_bits(v):
    return np.float64(v).view(np.uint64)


def check_record(dev, ref, where=""):
    for k in RESULT_KEYS:
        assert dev[k] == ref[k], (where, k, dev[k], ref[k])
    for k in SCORE_KEYS:
        assert f64_bits(dev[k]) == f64_bits(ref[k]), (where, k, dev[k], ref[k])


def check_pair(isc, i, j, d1, d2, where=""):
    geo, angle, inten, loop = R.pair(d1, d2)
    ok, dgeo, dinten = isc.is_loop_pair(i, j)
    ggeo, gangle = isc.calculate_geometry_dis(i, j)
    assert (gangle, ok) == (angle, loop), (where, gangle, angle, ok, loop)
    assert f64_bits(dgeo) == f64_bits(ggeo) == f64_bits(geo), (where, dgeo, geo)
    assert f64_bits(dinten) == f64_bits(inten), (where, dinten, inten)
    return angle


_routes = {}


def route(yaw):
    """The 102-keyframe loop route at one yaw offset: scans, poses, and the restatement's online records (computed once)."""
    if yaw not in _routes:
        scans, poses = isc_scene.route_keyframes(yaw_offset=math.radians(yaw))
        g = R.ISCGeneration()
        online = []
        for s, p in zip(scans, poses):
            g.makeAndSavedec(s, (p[0], p[1], 0.0))
            online.append((g.detectLoopClosureID(), g.last))
        assert sum(1 for _, r in online if r["loop_id"] != -1) == 23
        _routes[yaw] = {"scans": scans, "poses": poses, "g": g, "online": online}
    return _routes[yaw]


def device_cloud(lib, ctx, cloud):
    d = C.c_void_p()
    assert lib.ndt_device_alloc(ctx, max(16, cloud.nbytes), C.byref(d)) == 0
    if len(cloud):
        assert lib.ndt_memcpy_h2d(ctx, d, cloud.ctypes.data_as(C.c_void_p), cloud.nbytes) == 0
    return d


# points on the four axes (y = +-0 with x < 0 are both skipped), at the origin, at the f32 just below max_dis and at it,
# z at exactly its limits and one ulp outside, non-finite coordinates; intensities outside 0..1 and NaN
BELOW = np.nextafter(np.float32(40.0), np.float32(0.0))
EDGE_POINTS = np.array([
    [5.0, 0.0, 0.0, 0.5], [0.0, 5.0, 0.0, 0.6], [0.0, -5.0, 0.0, 0.7], [-5.0, 0.0, 0.0, 0.8], [-6.0, -0.0, 0.0, 0.9],
    [0.0, 0.0, 0.0, 0.3], [BELOW, 0.0, 1.0, 0.4], [40.0, 0.0, 1.0, 0.45], [0.0, BELOW, 1.0, 0.35], [-24.0, 32.0, 1.0, 0.2],
    [3.0, 4.0, np.float32(-0.9), 0.11], [3.0, 14.0, np.float32(30.0), 0.12],
    [13.0, 4.0, np.nextafter(np.float32(-0.9), np.float32(-1.0)), 0.13], [13.0, 14.0, np.nextafter(np.float32(30.0), np.float32(31.0)), 0.14],
    [np.nan, 1.0, 0.0, 0.5], [1.0, np.inf, 0.0, 0.5], [1.0, 1.0, np.nan, 0.5],
    [-20.0, 3.0, 0.0, -0.5], [-20.0, 13.0, 0.0, 1.5], [-20.0, 23.0, 0.0, np.nan], [20.0, -3.0, 0.0, np.inf],
    [21.0, 21.0, 0.0, 0.2], [21.0, 21.0, 0.0, 0.9], [21.0, 21.0, 0.0, 0.4],
], np.float32)


# ---------------------------------------------------------------------------------------------- descriptors
def test_abi_version():
    from xchu_slam_amd import _lib
    assert _lib.load().ndt_abi_version() == 6


def test_descriptors():
    """Clouds of 0, 1, 255, 256, 257 and 3000 points, the edge points, and 70 000 points (35 workgroups: the merge of the
    workgroups' cells), each added from the host and from a device pointer."""
    import xchu_slam_amd as xa
    scan = route(0.0)["scans"][7]
    poses = sc_scene.route_poses()
    from xchu_slam_amd import synth
    T = synth.pose_matrix(*poses[7])
    big = synth.sensor_scan(sc_scene.route_world(), T, 70000, 99)
    big = np.concatenate([big, isc_scene.reflectance(big.astype(np.float64) @ T[:3, :3].T + T[:3, 3])[:, None]], 1).astype(np.float32)
    assert len(big) == 70000
    clouds = [scan[:0], scan[100:101], scan[:255], scan[:256], scan[:257], scan, EDGE_POINTS, np.concatenate([scan, EDGE_POINTS]), big]
    with xa.ISCGeneration() as isc:
        assert isc.shape == (60, 60)
        for k, cl in enumerate(clouds):
            cl = np.ascontiguousarray(cl)
            ref = R.calculate_isc(cl)
            i = isc.makeAndSavedec(cl, (k, 0.0, 0.0))
            d = device_cloud(isc._lib, isc.ctx, cl)
            j = isc.makeAndSavedecDevice(d.value, len(cl), (k, 0.5, 0.0))
            assert (i + 1, len(isc)) == (j, j + 1)
            for slot in (i, j):
                got = isc.descriptor(slot)
                assert got.dtype == np.uint8 and np.array_equal(got, ref), (len(cl), slot, np.argwhere(got != ref)[:5])
            isc._lib.ndt_device_free(isc.ctx, d)
        assert not isc.descriptor(0).any() and np.count_nonzero(isc.descriptor(10)) > 100
        # known answers, independent of the restatement
        e = isc.descriptor(12)
        assert e[7, 45] == 153 and e[7, 14] == 178                  # +y and -y axes (0.6, 0.7)
        assert e[7, 59] == e[9, 59] == e[7, 0] == e[9, 0] == 0     # y = +-0, x < 0: both skipped
        assert e[59].tolist().count(0) == 58 and sorted(e[59][e[59] > 0].tolist()) == [89, 102]  # just below max_dis; 40.0 and (-24, 32) are not
        assert e[7, 8 + 30] == 28 and e[21, 12 + 30] == 30          # z at its limits is kept
        # ... and nothing else but +x, the origin, the clamped 1.5 and inf, and the duplicates' maximum
        assert sorted(e[e > 0].tolist()) == [28, 30, 76, 89, 102, 127, 153, 178, 229, 255, 255]
        # the position is narrowed through f32, the travel distance accumulates in f64
        p, t = isc.position(3)
        assert p.tolist() == [1.0, 0.5, 0.0] and t == 0.5 + math.sqrt(1.25) + 0.5
        rgb = isc.getLastISCRGB()
        assert rgb.shape == (60, 60, 3) and rgb.dtype == np.uint8 and np.array_equal(rgb, R.color_table()[isc.getLastISCMONO()])
        assert np.array_equal(isc.getLastISCMONO(), R.calculate_isc(big))


def test_descriptor_of_strided_records():
    """ndt_isc_add over 32-byte records with the intensity at float 4 (pcl::PointXYZI's layout, the padding poisoned)
    stores the bytes of the packed (N, 4) call."""
    import xchu_slam_amd as xa
    from xchu_slam_amd import _lib
    cloud = np.ascontiguousarray(np.concatenate([route(0.0)["scans"][7][:300], EDGE_POINTS]), np.float32)
    wide = np.full((len(cloud), 8), np.nan, np.float32)
    wide[:, :3] = cloud[:, :3]
    wide[:, 4] = cloud[:, 3]
    pos = (C.c_double * 3)(1.0, 2.0, 0.0)
    with xa.ISCGeneration() as isc:
        i = isc.makeAndSavedec(cloud, (1.0, 2.0, 0.0))
        idx = C.c_int(-1)
        st = isc._lib.ndt_isc_add(isc._handle, wide.ctypes.data_as(C.POINTER(C.c_float)), len(wide), 32, 4, pos, C.byref(idx))
        assert st == _lib.NDT_OK and idx.value == i + 1
        assert np.count_nonzero(isc.descriptor(i)) > 50
        assert np.array_equal(isc.descriptor(idx.value), isc.descriptor(i))


def test_second_shape():
    """20 rings x 90 sectors over 60 m: a row / column mix-up cannot survive a non-square descriptor."""
    import xchu_slam_amd as xa
    scan = np.concatenate([route(0.0)["scans"][30], EDGE_POINTS, np.float32([[0.0, 31.0, 0.0, 0.5], [59.0, 1.0, 0.0, 0.25]])])
    with xa.ISCGeneration(rings=20, sectors=90, max_dis=60.0) as isc:
        isc.makeAndSavedec(scan, (0, 0, 0))
        ref = R.calculate_isc(scan, 20, 90, 60.0)
        assert isc.descriptor(0).shape == (20, 90) and np.array_equal(isc.descriptor(0), ref)
        assert ref[10, 67] == 127 and ref[19, 45] == 63
        isc.add_descriptor(np.roll(ref, 80, axis=1), (0, 0, 0))
        assert np.array_equal(isc.descriptor(1), np.roll(ref, 80, axis=1))
        assert check_pair(isc, 0, 1, ref, np.roll(ref, 80, axis=1)) == 80
        # init_param reshapes an empty object only
        with pytest.raises(RuntimeError):
            isc.init_param(60, 60, 40.0)
    with xa.ISCGeneration() as isc:
        isc.init_param(20, 90, 60.0)
        isc.makeAndSavedec(scan, (0, 0, 0))
        assert np.array_equal(isc.descriptor(0), ref)
    for bad in (dict(rings=0), dict(rings=65), dict(sectors=19), dict(sectors=129), dict(max_dis=0.0)):
        with pytest.raises(xa._lib.NdtError):
            xa.ISCGeneration(**bad)


def test_database_growth():
    """70 adds cross the first growth step (64 slots): every earlier slot reads back as before."""
    import xchu_slam_amd as xa
    scan = route(0.0)["scans"][50]
    parts = [scan[40 * k: 40 * k + 40] for k in range(70)]
    refs = [R.calculate_isc(p) for p in parts]
    with xa.ISCGeneration() as isc:
        for k, p in enumerate(parts):
            if k % 7 == 3:
                isc.add_descriptor(refs[k], (k, 0, 0))
            else:
                isc.makeAndSavedec(p, (k, 0, 0))
            if k == 63:
                before = [isc.descriptor(s) for s in range(64)]
        assert len(isc) == 70
        for s in range(70):
            assert np.array_equal(isc.descriptor(s), refs[s]), s
            assert s >= 64 or np.array_equal(before[s], refs[s])
            p, t = isc.position(s)
            assert p.tolist() == [s, 0, 0] and t == float(s)
        # the masks moved too: a pair across the growth step
        check_pair(isc, 69, 5, refs[69], refs[5])
        check_pair(isc, 5, 66, refs[5], refs[66])


# ---------------------------------------------------------------------------------------------- is_loop_pair
def test_pairs_on_the_route():
    import xchu_slam_amd as xa
    for yaw, pairs in [(0.0, [(0, 0), (79, 1), (1, 79), (90, 12), (50, 10), (101, 22), (101, 0)]), (-45.0, [(79, 1), (1, 79), (95, 16), (60, 59)]),
                       (48.0, [(84, 6), (6, 84)])]:
        rt = route(yaw)
        descs = rt["g"].descs
        idx = sorted({k for pr in pairs for k in pr})
        with xa.ISCGeneration() as isc:
            for k in idx:
                isc.makeAndSavedec(rt["scans"][k], (0, 0, 0))
                assert np.array_equal(isc.descriptor(len(isc) - 1), descs[k])
            for i, j in pairs:
                angle = check_pair(isc, idx.index(i), idx.index(j), descs[i], descs[j], (yaw, i, j))
                for a in (angle, 0, 59, 30):
                    got = isc.calculate_intensity_dis(idx.index(i), idx.index(j), a)
                    assert f64_bits(got) == f64_bits(R.calculate_intensity_dis(descs[i], descs[j], a)), (yaw, i, j, a)
            with pytest.raises(xa._lib.NdtError):
                isc.is_loop_pair(0, len(idx))
            with pytest.raises(xa._lib.NdtError):
                isc.calculate_intensity_dis(0, 0, 60)


def test_pairs_handcrafted():
    """Column-rolled copies at every shift (angle >= 52 and angle < 10: the window wraps both ways), descriptors of only
    0 / 1 / 2, and shifts of equal count."""
    import xchu_slam_amd as xa
    rng = np.random.default_rng(11)
    base = route(0.0)["g"].descs[20]
    tri = rng.integers(0, 3, (60, 60)).astype(np.uint8)                 # only 0, 1, 2: the 2s never match
    periodic = np.zeros((60, 60), np.uint8)
    periodic[::3, ::5] = 1                                              # period 5: twelve equal shifts, the first wins
    periodic[1::3, ::5] = 77
    two = np.full((60, 60), 2, np.uint8)
    stored = [base, tri, periodic, two, np.zeros((60, 60), np.uint8), np.full((60, 60), 255, np.uint8), np.full((60, 60), 1, np.uint8)]
    with xa.ISCGeneration() as isc:
        for d in stored:
            isc.add_descriptor(d, (0, 0, 0))
        n0 = len(isc)
        for sh in range(60):
            isc.add_descriptor(np.roll(base, sh, axis=1), (0, 0, 0))
            isc.add_descriptor(np.roll(tri, sh, axis=1), (0, 0, 0))
        seen = set()
        for sh in range(60):
            a = check_pair(isc, 0, n0 + 2 * sh, base, np.roll(base, sh, axis=1), ("base", sh))
            b = check_pair(isc, 1, n0 + 2 * sh + 1, tri, np.roll(tri, sh, axis=1), ("tri", sh))
            assert a == b == sh
            seen.add(a)
            assert isc.is_loop_pair(0, n0 + 2 * sh)[0] and isc.is_loop_pair(0, n0 + 2 * sh)[2] == 1.0
        assert seen == set(range(60))
        for i in range(len(stored)):
            for j in range(len(stored)):
                check_pair(isc, i, j, stored[i], stored[j], (i, j))
        assert isc.calculate_geometry_dis(2, 2) == (3360 / 3600, 0)     # 3120 zeros and 240 ones; the 77s never match
        assert isc.calculate_geometry_dis(3, 3) == (0.0, 0)             # identical, and nothing matches
        assert isc.is_loop_pair(4, 4) == (True, 1.0, 1.0) and isc.is_loop_pair(6, 6) == (True, 1.0, 1.0)
        assert isc.is_loop_pair(4, 5) == (False, 0.0, 0.0)              # the full-scale SAD: 1 - 1.0


# ---------------------------------------------------------------------------------------------- detection
@pytest.mark.parametrize("yaw", YAWS)
def test_detection_online_and_batch(yaw):
    """add then detect per keyframe, and all 102 keyframes in one launch: every field of every record equals the
    restatement's, and the two agree."""
    import xchu_slam_amd as xa
    rt = route(yaw)
    with xa.ISCGeneration() as isc:
        online = []
        for q, (s, p) in enumerate(zip(rt["scans"], rt["poses"])):
            assert isc.makeAndSavedec(s, (p[0], p[1], 0.0)) == q
            got = isc.detectLoopClosureID()
            ref_pair, ref = rt["online"][q]
            assert got == (ref_pair[0], float(ref_pair[1])), (q, got, ref_pair)
            check_record(isc.last_result(), ref, f"keyframe {q}")
            online.append(isc.last_result())
        assert np.array_equal(isc.descriptor(57), rt["g"].descs[57])
        p, t = isc.position(101)
        assert p.tolist() == rt["g"].pos[101] and t == rt["g"].travel[101]
        batch = isc.detect_batch(np.arange(102))
        assert batch == online
        assert isc.detect_batch([101, 3, 80]) == [online[101], online[3], online[80]] and isc.detect_batch([]) == []
        with pytest.raises(xa._lib.NdtError):
            isc.detect_batch([102])
    dev = xa.detect_loops_isc(rt["scans"], rt["poses"])
    assert dev == online
    loops = [r for r in dev if r["loop_id"] != -1]
    assert [r["curr_id"] for r in loops] == list(range(79, 102))
    assert {r["angle"] for r in loops} == {0.0: {0}, 48.0: {8}, -45.0: {52, 53}}[yaw]


def zigzag_positions(n):
    """Keyframe k at the origin (k even) or 30 m away (k odd): the even ones gate each other, and an odd one the even
    ones more than 33 keyframes back."""
    return [(30.0 * (k % 2), 0.0, 0.0) for k in range(n)]


def test_detection_handcrafted():
    """40 descriptors through add_descriptor: two candidates of equal sum (the lower index wins), a best candidate at
    index 0 beside a weaker passing one (no loop), a query with no gated pair; twice, bitwise equal."""
    import xchu_slam_amd as xa
    rng = np.random.default_rng(2)
    A = route(0.0)["g"].descs[30]
    weaker = A.copy()
    dim = tuple(np.argwhere(A > 3)[:40].T)
    weaker[dim] = A[dim] // 2 + 2      # the same geometry, a little intensity off
    B = route(0.0)["g"].descs[70]
    descs = [rng.integers(0, 256, (60, 60)).astype(np.uint8) for _ in range(40)]
    descs[0] = A
    descs[2] = weaker
    descs[4] = A                       # query 4: candidates 0 (A itself) and 2 (weaker): the winner is index 0
    descs[10] = B
    descs[12] = np.roll(B, 7, axis=1)
    descs[14] = B
    descs[16] = np.roll(B, 55, axis=1)  # query 16: candidates 10, 12, 14 score the same, the lowest index wins
    descs[38] = np.roll(A, 3, axis=1)   # query 38: index 0 and 4 tie, 2 passes lower: index 0 wins, so no loop
    pos = zigzag_positions(40)
    g = R.ISCGeneration()
    for d, p in zip(descs, pos):
        g.add_descriptor(d, p)
    ref = [g.detect(q) for q in range(40)]
    # (a descriptor against itself scores 1.0 in intensity and, in geometry, its share of cells that are 0 or 1)
    assert (ref[4]["loop_id"], ref[4]["best_id"], ref[4]["n_loop_pairs"], ref[4]["inten_score"]) == (-1, 0, 2, 1.0)
    assert (ref[16]["loop_id"], ref[16]["inten_score"], ref[16]["angle"]) == (10, 1.0, 5) and ref[16]["n_loop_pairs"] >= 3
    assert (ref[38]["loop_id"], ref[38]["best_id"], ref[38]["inten_score"], ref[38]["angle"]) == (-1, 0, 1.0, 57) and ref[38]["n_loop_pairs"] >= 3
    assert ref[1]["n_gated"] == 0 and ref[39]["n_gated"] > 19 and ref[14]["loop_id"] == 10
    with xa.ISCGeneration() as isc:
        for d, p in zip(descs, pos):
            isc.add_descriptor(d, p)
        first = isc.detect_batch(np.arange(40))
        for q in range(40):
            check_record(first[q], ref[q], f"descriptor {q}")
        assert isc.detect_batch(np.arange(40)) == first
        isc.detectLoopClosureID()
        assert isc.last_result() == first[39]


def test_detection_over_several_chunks():
    """300 small descriptors (4 rings x 20 sectors, drawn from six patterns with a few cells changed): a query's
    candidates span two 256-candidate workgroups and the database grows three times."""
    import xchu_slam_amd as xa
    rng = np.random.default_rng(8)
    pool = [rng.choice(np.array([0, 0, 1, 1, 1, 60, 200], np.uint8), (4, 20)) for _ in range(6)]
    descs = []
    for k in range(300):
        d = np.roll(pool[rng.integers(0, 6)], int(rng.integers(0, 20)), axis=1).copy()
        d[rng.integers(0, 4), rng.integers(0, 20)] = rng.integers(0, 256)
        descs.append(d)
    pos = [(30.0 * (k % 2) + 0.25 * (k % 5), 0.5 * (k % 3), 0.0) for k in range(300)]
    prm = dict(rings=4, sectors=20, max_dis=40.0)
    g = R.ISCGeneration(**prm)
    for d, p in zip(descs, pos):
        g.add_descriptor(d, p)
    query = [299, 298, 257, 256, 255, 254, 100, 1, 0]
    ref = [g.detect(q) for q in query]
    assert ref[0]["n_gated"] > 140 and ref[0]["n_loop_pairs"] > 0 and ref[0]["loop_id"] > 0
    dev = xa.detect_loops_isc(descriptors=descs, poses=pos, **prm)
    assert len(dev) == 300
    for q, r in zip(query, ref):
        check_record(dev[q], r, f"descriptor {q}")


# ---------------------------------------------------------------------------------------------- integration
def test_shares_a_registration_context():
    """An NDT registration, an SCManager and an ISCGeneration on one context: all three keep working."""
    import xchu_slam_amd as xa
    from helpers import small_pair
    rt = route(0.0)
    pair = small_pair(seed=3, n_source=1000)
    with xa.NormalDistributionsTransform() as ndt:
        ndt.setInputTarget(pair.target)
        ndt.setInputSource(pair.source)
        ndt.align(pair.guess)
        T = ndt.getFinalTransformation()
        sc = xa.SCManager(registration=ndt)
        isc = xa.ISCGeneration(registration=ndt)
        assert isc.registration is ndt and isc.ctx is ndt.ctx
        for i in (1, 40, 79):
            sc.makeAndSaveScancontextAndKeys(rt["scans"][i][:, :3])
            isc.makeAndSavedec(rt["scans"][i], rt["g"].pos[i])
        sc0 = sc.polarcontext(2)
        assert np.array_equal(isc.descriptor(2), rt["g"].descs[79]) and len(isc) == 3 and len(sc) == 3
        # keyframe 79 against 1 and 40 alone: the travel distance between them is the straight chord here
        one = R.ISCGeneration()
        for i in (1, 40, 79):
            one.add_descriptor(rt["g"].descs[i], rt["g"].pos[i])
        isc.detectLoopClosureID()
        check_record(isc.last_result(), one.detect(2))
        ndt.align(pair.guess)
        assert np.array_equal(ndt.getFinalTransformation().view(np.uint32), T.view(np.uint32))
        assert sc.detectLoopClosureID()[0] == -1 and np.array_equal(sc.polarcontext(2), sc0)
        check_pair(isc, 2, 0, rt["g"].descs[79], rt["g"].descs[1])
        isc.close()
        sc.close()
        ndt.align(pair.guess)
        assert np.array_equal(ndt.getFinalTransformation().view(np.uint32), T.view(np.uint32))


N_CLOSE = 90   # keyframes of the route handed to close_loops: the revisits 79 .. 89
REFINE = dict(search_num=25, leaf=0.5)


def compose(records, keyframes, poses):
    import xchu_slam_amd as xa
    accepted, rejected = [], []
    for curr, rec in enumerate(records):
        prev = rec["loop_id"]
        if prev == -1:
            continue
        if math.sqrt((poses[prev][0] - poses[curr][0]) ** 2 + (poses[prev][1] - poses[curr][1]) ** 2) > 20.0:
            rejected.append((prev, curr, "pair_distance"))
            continue
        out = xa.refine_loop(keyframes, poses, prev, curr, **REFINE)
        if out["accepted"]:
            accepted.append((prev, curr, out["transform"], out["score"]))
        else:
            rejected.append((prev, curr, "icp"))
    return accepted, rejected


def same_closures(a, b):
    (acc_a, rej_a), (acc_b, rej_b) = a, b
    assert rej_a == rej_b and [(x[0], x[1], x[3]) for x in acc_a] == [(x[0], x[1], x[3]) for x in acc_b]
    for x, y in zip(acc_a, acc_b):
        assert np.array_equal(np.asarray(x[2]).view(np.uint32), np.asarray(y[2]).view(np.uint32))


def test_close_loops_with_isc():
    import xchu_slam_amd as xa
    rt = route(0.0)
    keyframes, poses = rt["scans"][:N_CLOSE], rt["poses"][:N_CLOSE]
    records = xa.detect_loops_isc(keyframes, poses)
    assert [r["curr_id"] for r in records if r["loop_id"] != -1] == list(range(79, N_CLOSE))
    got = xa.close_loops(keyframes, poses, loop_method=2, **REFINE)
    same_closures(got, compose(records, keyframes, poses))
    assert len(got[0]) >= 1 and len(got[0]) + len(got[1]) == N_CLOSE - 79
    gated = xa.close_loops(keyframes, poses, max_pair_dist=-1.0, loop_method=2, **REFINE)
    assert not gated[0] and [r[2] for r in gated[1]] == ["pair_distance"] * (N_CLOSE - 79)
    with pytest.raises(ValueError):
        xa.close_loops(keyframes, poses, loop_method=3)


def test_close_loops_default_is_unchanged():
    """Without loop_method, close_loops is what it was: detect_loops, the gate, refine_loop."""
    import xchu_slam_amd as xa
    rt = route(0.0)
    keyframes, poses = rt["scans"][:N_CLOSE], rt["poses"][:N_CLOSE]
    detect = dict(dist_thres=0.4, tree_making_period=1)
    records = xa.detect_loops([k[:, :3] for k in keyframes], **detect)
    assert sum(1 for r in records if r["loop_id"] != -1) >= 5
    want = compose(records, keyframes, poses)
    same_closures(xa.close_loops(keyframes, poses, detect_args=detect, **REFINE), want)
    same_closures(xa.close_loops(keyframes, poses, detect_args=detect, loop_method=1, **REFINE), want)
