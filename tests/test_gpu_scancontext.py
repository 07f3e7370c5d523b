"""Scan Context on the device (xa.SCManager, xa.detect_loops, xa.close_loops) against tests/sc_restate.py, bitwise
unless said otherwise.

The device's f64 arctangent and numpy's need not agree to the last bit: a scan is compared only under the restatement's
input condition that no point changes its bin when the arctangent moves by +-4 ulp before it is narrowed to f32 or when
r moves by one f32 ulp (sc_restate.bin_sensitive); points placed on an edge on purpose are exact by construction (their
r and quotient are exact) and are listed where they are used.  Ring-key neighbours at an equal distance go to the lower
index on both sides; the route's queries are asserted to have none.
"""
import ctypes as C

import numpy as np
import pytest

import sc_restate as R
import sc_scene

pytestmark = pytest.mark.gpu

REVISIT = 79   # keyframe q sees the place of keyframe q - 79 again


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_record(dev, ref, where=""):
    for k in ("loop_id", "nn_idx", "nn_align", "cand_idx", "cand_shift"):
        assert dev[k] == ref[k], (where, k, dev[k], ref[k])
    assert same_bits(np.float64(dev["min_dist"]), np.float64(ref["min_dist"])), (where, dev["min_dist"], ref["min_dist"])
    assert same_bits(np.array(dev["cand_dist"], np.float64), np.array(ref["cand_dist"], np.float64)), (where, dev["cand_dist"], ref["cand_dist"])
    assert same_bits(np.float32(dev["yaw_diff"]), np.float32(ref["yaw_diff"])), (where, dev["yaw_diff"], ref["yaw_diff"])


@pytest.fixture(scope="module")
def route():
    """The 102-keyframe loop route (3000-point scans), its restated descriptors and the restatement's online records
    (default parameters: period 30, 3 candidates, 10 % of the shifts)."""
    scans, poses = sc_scene.route_keyframes(3000)
    assert len(scans) == 102
    for s in scans:
        assert len(R.bin_sensitive(s)) == 0, "input condition: no bin-sensitive point"
    m = R.SCManager()
    online = []
    for s in scans:
        m.makeAndSaveScancontextAndKeys(s)
        m.detectLoopClosureID()
        online.append(m.last)
    assert not any(r["tie"] for r in online), "input condition: no equal ring-key or candidate distances"
    return {"scans": scans, "poses": poses, "descs": m.descs, "online": online, "cache": {}}


# ---------------------------------------------------------------------------------------------- descriptor and keys
EDGE_POINTS = np.array([
    [0.0, 7.0, 0.3], [9.0, 0.0, 0.4], [-11.0, 0.0, 0.5], [0.0, -13.0, 0.6],   # the axes
    [80.0, 0.0, 1.0], [0.0, 80.0, 1.1], [-48.0, 64.0, 1.2],                    # r == 80 exactly: kept, ring 20
    [0.0, 0.0, 2.5],                                                           # r == 0: ring 1, sector 1
    [4.0, 0.0, 0.7], [0.0, 8.0, 0.8],                                          # r on a ring edge, exactly
], np.float32)


def full_scan():
    """5000 street-scene points plus the axis and edge points, points beyond 80 m, negative heights (one bin's only
    points below -2, one under NO_POINT) and duplicates within one bin."""
    world = sc_scene.route_world()
    from xchu_slam_amd import synth
    scan = synth.sensor_scan(world, synth.pose_matrix(*sc_scene.route_poses()[7]), 5000, 99, max_range=60.0)
    beyond = np.array([[np.nextafter(np.float32(80.0), np.float32(90.0)), 0.0, 3.0], [70.0, 70.0, 1.0], [-200.0, 5.0, 0.5],
                       [0.0, 80.01, 2.0]], np.float32)
    negative = np.array([[75.5, 3.0, -4.0], [75.6, 3.1, -7.5], [77.0, -20.0, -1500.0], [30.0, 30.5, -1.99]], np.float32)
    dup = np.array([[20.0, 20.0, 1.0]] * 5 + [[20.0, 20.0, 1.5]] * 3, np.float32)
    random_part = np.concatenate([scan, beyond, negative, dup]).astype(np.float32)
    random_part = np.delete(random_part, R.bin_sensitive(random_part), axis=0)   # (empty for this seed)
    cloud = np.concatenate([random_part, EDGE_POINTS]).astype(np.float32)
    # the only points a one-ulp move of r would change are the five placed exactly on r == 80 or on a ring edge
    sens = R.bin_sensitive(cloud)
    assert set(sens.tolist()) == {len(random_part) + k for k in (4, 5, 6, 8, 9)}, sens
    return cloud


def device_cloud(lib, ctx, cloud):
    from xchu_slam_amd import synth
    xyz4 = synth.to_xyz4(cloud)
    d = C.c_void_p()
    assert lib.ndt_device_alloc(ctx, max(16, xyz4.nbytes), C.byref(d)) == 0
    if len(xyz4):
        assert lib.ndt_memcpy_h2d(ctx, d, xyz4.ctypes.data_as(C.c_void_p), xyz4.nbytes) == 0
    return d


def test_descriptor_and_keys():
    """Scans of 0, 1, 257 and 5000+ points (no launch, a partial workgroup, a partial grid, three workgroups), each added
    from the host and from a device pointer."""
    import xchu_slam_amd as xa
    cloud = full_scan()
    assert len(cloud) > 2 * 2048
    clouds = [cloud[:0], cloud[100:101], cloud[:257], cloud]
    with xa.SCManager() as sc:
        for cl in clouds:
            ref = R.make_scancontext(cl)
            i = sc.makeAndSaveScancontextAndKeys(cl)
            d = device_cloud(sc._lib, sc.ctx, cl)
            j = sc.makeAndSaveScancontextAndKeysDevice(d.value, len(cl))
            assert (i + 1, len(sc)) == (j, j + 1)
            for slot in (i, j):
                assert same_bits(sc.polarcontext(slot), ref), (len(cl), slot)
                assert same_bits(sc.ringkey(slot), R.ring_key(ref))
                assert same_bits(sc.sectorkey(slot), R.sector_key(ref))
            sc._lib.ndt_device_free(sc.ctx, d)
        assert not sc.polarcontext(0).any()
        # pcl::PointXYZI records (32-byte stride) take the same path as an (N, 3) array
        rec = np.zeros(len(cloud), xa.ndt.POINT_XYZI_DTYPE)
        rec["x"], rec["y"], rec["z"], rec["intensity"] = cloud[:, 0], cloud[:, 1], cloud[:, 2], 0.5
        k = sc.makeAndSaveScancontextAndKeys(rec)
        assert same_bits(sc.polarcontext(k), sc.polarcontext(k - 1)) and same_bits(sc.ringkey(k), sc.ringkey(k - 1))
        full = sc.getConstRefRecentSCD()
        # known answers, independent of the restatement: the axis and edge points own their bins' maxima
        assert full[1, 14] >= np.float32(2.3) and full[19, 0] == float(np.float32(np.float64(np.float32(1.0)) + 2.0))
        assert full[0, 0] >= 4.5 and full[19, 14] >= float(np.float32(3.1))
        # the bin whose only points are below the sensor keeps its (negative) maximum; the one under NO_POINT stays 0
        r, s, _, _ = R._bins(np.float32([75.5, 77.0]), np.float32([3.0, -20.0]))
        assert full[r[0] - 1, s[0] - 1] == -2.0 and full[r[1] - 1, s[1] - 1] == 0.0
        # a descriptor stored as is takes the same keys
        k = sc.saveScancontextAndKeys(full)
        assert same_bits(sc.polarcontext(k), full) and same_bits(sc.ringkey(k), sc.ringkey(k - 1))
        assert same_bits(sc.sectorkey(k), sc.sectorkey(k - 1))
        assert sc.distanceBtnScanContext(k, k - 1) == R.distance(full, full)


def test_database_growth(route):
    """70 adds cross the first growth step (64 slots): every earlier slot reads back as before."""
    import xchu_slam_amd as xa
    scan = route["scans"][50]
    parts = [scan[40 * k: 40 * k + 40] for k in range(70)]
    refs = [R.make_scancontext(p) for p in parts]
    with xa.SCManager() as sc:
        for k, p in enumerate(parts):
            if k % 7 == 3:
                sc.saveScancontextAndKeys(refs[k])
            else:
                sc.makeAndSaveScancontextAndKeys(p)
            if k == 63:
                before = [sc._get(s) for s in range(64)]
        assert len(sc) == 70
        for s in range(70):
            got = sc._get(s)
            for a, b in zip(got, (refs[s], R.ring_key(refs[s]), R.sector_key(refs[s]))):
                assert same_bits(a, b), s
            assert s >= 64 or all(same_bits(a, b) for a, b in zip(got, before[s])), s
        # the column norms moved too: a pair on each side of the growth step and one across it
        for i, j in ((5, 20), (66, 69), (69, 5)):
            dist, shift = sc.distanceBtnScanContext(i, j)
            rd, rs = R.distance(refs[i], refs[j])
            assert same_bits(np.float64(dist), np.float64(rd)) and shift == rs, (i, j, dist, shift, rd, rs)


# ---------------------------------------------------------------------------------------------- distanceBtnScanContext
def test_distance_pairs(route):
    import xchu_slam_amd as xa
    d = route["descs"]
    gaps = d[3].copy()
    gaps[:, 5:20] = 0.0
    gaps[:, 50:] = 0.0
    stored = [d[0], d[1], d[40], d[80], np.roll(d[0], 1, axis=1), np.roll(d[0], 29, axis=1), np.roll(d[0], 59, axis=1), gaps,
              np.zeros((20, 60)), d[3]]
    pairs = [(0, 0), (0, 1), (1, 0), (0, 2), (3, 0), (0, 4), (4, 0), (0, 5), (6, 0), (7, 9), (9, 7), (8, 0), (0, 8), (8, 8), (7, 8)]
    with xa.SCManager() as sc:
        for x in stored:
            sc.saveScancontextAndKeys(x)
        for ratio in (0.1, 1.0):
            sc.set_params(search_ratio=ratio)
            for i, j in pairs:
                dist, shift = sc.distanceBtnScanContext(i, j)
                rd, rs = R.distance(stored[i], stored[j], ratio)
                assert same_bits(np.float64(dist), np.float64(rd)) and shift == rs, (ratio, i, j, dist, shift, rd, rs)
        assert sc.distanceBtnScanContext(0, 4)[1] == 59 and sc.distanceBtnScanContext(6, 0)[1] == 59
        assert sc.distanceBtnScanContext(0, 8) == (R.BIG, 0)   # every shift's NaN loses: the initial minimum, shift 0
        with pytest.raises(xa._lib.NdtError):
            sc.distanceBtnScanContext(0, len(stored))


def test_shares_a_registration_context(route):
    """An SCManager on an existing registration's context (its device and stream) leaves that registration usable, and
    is closed before it."""
    import xchu_slam_amd as xa
    from helpers import small_pair
    pair = small_pair(seed=3, n_source=1000)
    with xa.NormalDistributionsTransform() as ndt:
        ndt.setInputTarget(pair.target)
        ndt.setInputSource(pair.source)
        ndt.align(pair.guess)
        T = ndt.getFinalTransformation()
        sc = xa.SCManager(registration=ndt)
        assert sc.registration is ndt and sc.ctx is ndt.ctx
        for i in (0, 40, 80):
            sc.makeAndSaveScancontextAndKeys(route["scans"][i])
        assert same_bits(sc.polarcontext(2), route["descs"][80]) and len(sc) == 3
        assert sc.detectLoopClosureID() == (-1, 0.0) and sc.last_result()["cand_idx"] == []
        sc.close()
        ndt.align(pair.guess)
        assert same_bits(ndt.getFinalTransformation(), T)


# ---------------------------------------------------------------------------------------------- online detection
@pytest.mark.parametrize("thres", [0.2, 0.4])
def test_online_detection(route, thres):
    """detectLoopClosureID after every add: the early return (30 calls), then 1 searchable key for 30 calls (a stale set),
    31 for the next 30, 61 for the rest.  The threshold only changes loop_id: revisit distances are 0.22-0.33 here and
    the others at least 0.43 (restatement), so 0.2 finds nothing and 0.4 the revisits."""
    import xchu_slam_amd as xa
    ref = []
    for r in route["online"]:
        r = dict(r)
        r["loop_id"] = r["nn_idx"] if r["cand_idx"] and r["min_dist"] < thres else -1
        ref.append(r)
    loops = [(q, r["nn_idx"]) for q, r in enumerate(ref) if r["loop_id"] != -1]
    if thres == 0.2:
        assert not loops
    else:
        assert sum(1 for q, i in loops if abs(i - (q - REVISIT)) <= 2) >= 15, loops
    assert [len(r["cand_idx"]) for r in ref[28:34]] == [0, 0, 1, 1, 1, 1] and len(ref[60]["cand_idx"]) == 3
    with xa.SCManager() as sc:
        sc.setSCdistThres(thres)
        for q, scan in enumerate(route["scans"]):
            assert sc.makeAndSaveScancontextAndKeys(scan) == q
            loop_id, yaw = sc.detectLoopClosureID()
            dev = sc.last_result()
            check_record(dev, ref[q], f"keyframe {q}")
            assert (loop_id, yaw) == (dev["loop_id"], dev["yaw_diff"])
        assert same_bits(sc.polarcontext(57), route["descs"][57])


# ---------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("period,cands,ratio", [(30, 3, 0.1), (1, 3, 0.1), (1, 10, 0.1), (30, 10, 1.0), (1, 3, 1.0), (30, 3, 1.0),
                                                (30, 10, 0.1), (1, 10, 1.0)])
def test_detect_loops(route, period, cands, ratio):
    import xchu_slam_amd as xa
    prm = dict(num_candidates=cands, search_ratio=ratio, dist_thres=0.4)
    ref = R.detect_loops(route["descs"], tree_making_period=period, cache=route["cache"], **prm)
    assert not any(r["tie"] for r in ref), "input condition: no equal ring-key or candidate distances"
    dev = xa.detect_loops(route["scans"], tree_making_period=period, **prm)
    assert len(dev) == len(ref) == 102
    for q in range(102):
        check_record(dev[q], ref[q], f"keyframe {q}")
    if (period, cands, ratio) == (30, 3, 0.1):
        for q in range(102):   # the online run's records, up to the threshold
            assert dev[q]["cand_idx"] == route["online"][q]["cand_idx"] and dev[q]["cand_dist"] == route["online"][q]["cand_dist"]
    if cands == 10:
        assert max(len(r["cand_idx"]) for r in dev) == 10 and len(dev[35]["cand_idx"]) == (6 if period == 1 else 1)


def test_detect_loops_handcrafted_ties(route):
    """34 descriptors through saveScancontextAndKeys: 3 and 1 are identical (equal ring-key distances to every query),
    2 is the zero descriptor, and the last is a rolled copy of both twins.  The lower-index rule decides."""
    import xchu_slam_amd as xa
    descs = [route["descs"][i] for i in range(0, 68, 2)]
    descs[3] = descs[1]
    descs[2] = np.zeros((20, 60))
    descs[33] = np.roll(descs[1], 5, axis=1)
    assert len(descs) == 34
    prm = dict(num_candidates=3, num_exclude_recent=30, dist_thres=0.4)
    ref = R.detect_loops(descs, tree_making_period=1, **prm)
    assert ref[33]["tie"] and ref[33]["cand_idx"][:2] == [1, 3] and ref[33]["loop_id"] == 1 and ref[33]["nn_align"] == 5
    dev = xa.detect_loops(descriptors=descs, tree_making_period=1, **prm)
    for q in range(34):
        check_record(dev[q], ref[q], f"descriptor {q}")
    with xa.SCManager(num_exclude_recent=0, num_candidates=16, tree_making_period=1) as sc:
        for x in descs[:5]:
            sc.saveScancontextAndKeys(x)
        # the query itself is searchable with nothing excluded; the zero descriptor is a candidate that never wins
        rec = sc.detect_batch([4, 4, 0], [5, 0, 1])
        one = R.detect_one(descs[:5], [R.ring_key(x) for x in descs[:5]], 4, 5, num_candidates=16)
        check_record(rec[0], one)
        assert rec[0]["cand_idx"][0] == 4 and sorted(rec[0]["cand_idx"]) == [0, 1, 2, 3, 4]
        assert rec[0]["cand_dist"][rec[0]["cand_idx"].index(2)] == R.BIG
        assert rec[1] == sc.detect_batch([4], [-3])[0] and rec[1]["loop_id"] == -1 and rec[1]["cand_idx"] == []
        with pytest.raises(xa._lib.NdtError):
            sc.detect_batch([5], [1])
        with pytest.raises(xa._lib.NdtError):
            sc.set_params(num_candidates=17)
        with pytest.raises(xa._lib.NdtError):
            sc.set_params(num_candidates=3, search_ratio=1.5)


# ---------------------------------------------------------------------------------------------- close_loops
def test_close_loops():
    """The route with 4200-point keyframes and ground-truth poses perturbed as helpers.small_pair perturbs its guess
    (0.3 m, 0.3 m, 0.05 m, 0.5, 0.5, 1.0 deg).  Target submaps are pgo_node's +-25 keyframes: these scans are sparse
    random samples of the scene (0.2 points / m^2 on the ground), and against a submap of five of them the fitness score
    of even a perfect alignment is above the 0.3 gate (0.35-0.46, CPU estimate); against +-25 it is 0.08-0.15."""
    import xchu_slam_amd as xa
    scans, truth = sc_scene.route_keyframes(4200)
    scans = [np.delete(s, R.bin_sensitive(s), axis=0) for s in scans]   # input condition (one point of 428 400 here)
    rng = np.random.default_rng(17)
    keyframes = [np.concatenate([s, rng.uniform(0, 1, (len(s), 1)).astype(np.float32)], 1) for s in scans]
    amp = np.array([0.3, 0.3, 0.05, np.radians(0.5), np.radians(0.5), np.radians(1.0)])
    poses = [tuple(np.array(p) + rng.uniform(-1, 1, 6) * amp) for p in truth]
    detect = dict(dist_thres=0.4, tree_making_period=1)
    refine = dict(search_num=25, leaf=0.5)
    ref = R.detect_loops([R.make_scancontext(s) for s in scans], **detect)
    assert not any(r["tie"] for r in ref)
    found = [(r["loop_id"], q) for q, r in enumerate(ref) if r["loop_id"] != -1]
    gate = [bool(np.hypot(poses[i][0] - poses[q][0], poses[i][1] - poses[q][1]) <= 20.0) for i, q in found]
    assert len(found) >= 15 and all(gate)   # a revisit is within a few metres of its match
    accepted, rejected = xa.close_loops(keyframes, poses, detect_args=detect, **refine)
    # every pair handed to ICP is a pair the restatement detects (all pass the 20 m gate here)
    assert sorted([(a[0], a[1]) for a in accepted] + [(r[0], r[1]) for r in rejected]) == sorted(found)
    assert all(r[2] == "icp" for r in rejected)
    assert len(accepted) >= 1
    for loop_idx, curr_idx, T, score in accepted:
        one = xa.refine_loop(keyframes, poses, loop_idx, curr_idx, **refine)
        assert one["accepted"] and same_bits(one["transform"], T) and one["score"] == score
    # the gate alone: nothing is closer than 0 m, so nothing reaches ICP
    accepted0, rejected0 = xa.close_loops(keyframes, poses, max_pair_dist=-1.0, detect_args=detect, **refine)
    assert not accepted0 and sorted((r[0], r[1]) for r in rejected0) == sorted(found)
    assert all(r[2] == "pair_distance" for r in rejected0)
