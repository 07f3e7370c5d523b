"""The ground detection's restatement (tests/ground_restate.py) against what is known independently of it: the
generator's published outputs, the sampler's rules replayed over a materialised index array, the RANSAC rule computed by
hand from the hypotheses' counts, and the node's gates and quirks on constructed clouds.  No GPU."""
import math

import numpy as np
import pytest

import ground_restate as gr
import ground_scene as gs

F32 = np.float32


# ------------------------------------------------------------------------------------------------ generator
def test_mt19937_default_seed_10000th_output():
    g = gr.MT19937()  # seed 5489: the value the C++ standard quotes for mt19937
    w = g.words(10000)
    assert int(w[-1]) == 4123659995


def test_mt19937_seed_12345_is_numpys_raw_stream():
    rs = np.random.RandomState(gr.SEED)
    assert list(rs.get_state()[1]) == gr.MT19937(gr.SEED).mt  # init_genrand
    want = rs.randint(0, 2 ** 32, size=2000, dtype=np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(gr.MT19937(gr.SEED).words(2000), want)


def test_rnd_is_the_word_shifted_right_by_one():
    a, b = gr.MT19937(gr.SEED), gr.MT19937(gr.SEED)
    for _ in range(100):
        r = gr.rnd(a)
        assert r == b.next() >> 1 and 0 <= r <= gr.INT_MAX


# ------------------------------------------------------------------------------------------------ sampler
def _dense_samples(pts, count):
    """drawIndexSample over a materialised shuffled_indices_, isSampleGood redraws included."""
    n = len(pts)
    arr, gen, out = list(range(n)), gr.MT19937(gr.SEED), []
    while len(out) < count:
        for i in range(3):
            j = i + gr.rnd(gen) % (n - i)
            arr[i], arr[j] = arr[j], arr[i]
        if not gr.collinear(pts[arr[0]], pts[arr[1]], pts[arr[2]]):
            out.append(tuple(arr[:3]))
    return out


def test_sampler_triples_are_distinct_and_follow_the_persistent_shuffle():
    pts = gs.scene(1)[:700]
    s = gr.Sampler(pts)
    got = [s.sample() for _ in range(200)]
    assert all(len(set(t)) == 3 and all(0 <= v < len(pts) for v in t) for t in got)
    assert got == _dense_samples(pts, 200)
    assert len(s.shuffled) <= 3 + s.draws  # only touched positions are kept
    # sample i + 1 depends on sample i's swaps: over a small cloud, where draws meet touched positions, a sampler that
    # forgets its swaps between samples (same generator words) leaves the sequence, the persistent one stays on it
    small = np.random.default_rng(0).uniform(-5, 5, (9, 4)).astype(F32)
    keeps, forgets = gr.Sampler(small), gr.Sampler(small)
    a, b = [], []
    for _ in range(20):
        a.append(keeps.sample())
        forgets.shuffled = {}
        b.append(forgets.sample())
    assert a == _dense_samples(small, 20) and a != b and a[0] == b[0]


def _line_cloud():
    """47 points on a line (exactly: small integers) and 3 off it."""
    i = np.arange(47, dtype=np.float64)
    line = np.column_stack([i, 2 * i, 3 * i, np.zeros(47)])
    off = np.array([[0.5, 7.0, -3.0, 0], [11.0, -2.0, 4.5, 0], [-6.0, 1.0, 9.0, 0]])
    return np.concatenate([line, off]).astype(F32)


def test_sampler_redraws_a_collinear_triple():
    pts = _line_cloud()
    assert gr.collinear(pts[3], pts[17], pts[40]) and not gr.collinear(pts[3], pts[17], pts[48])
    s = gr.Sampler(pts)
    got = [s.sample() for _ in range(30)]
    assert all(not gr.collinear(*pts[list(t)]) for t in got)
    assert s.draws > 3 * len(got)  # some draws were thrown away
    assert got == _dense_samples(pts, 30)


# ------------------------------------------------------------------------------------------------ RANSAC
def _known_plane(seed=3, n_in=800, n_out=200, noise=0.02):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-15, 15, (n_in, 2))
    a = np.column_stack([xy, gs.GROUND_Z + rng.uniform(-noise, noise, n_in)])
    b = np.column_stack([rng.uniform(-15, 15, (n_out, 2)), rng.uniform(-1.2, 0.4, n_out)])
    pts = np.concatenate([a, b])
    perm = rng.permutation(len(pts))
    return pts[perm].astype(F32), np.flatnonzero(perm < n_in)


def test_ransac_iterations_follow_the_rule_and_the_plane_is_within_the_noise():
    pts, ground = _known_plane()
    r = gr.ransac(pts)
    # the rule by hand, from the hypotheses' counts alone
    logp, best, k, it = math.log(1 - 0.99), -1, 1.0, 0
    for _, coef, count, status in r["hypotheses"]:
        assert status == 1
        if count > best:
            best = count
            w = count / len(pts)
            k = logp / math.log(min(1 - gr.DBL_EPS, max(gr.DBL_EPS, 1 - w * w * w)))
        it += 1
        if not it < k:
            break
    assert it == len(r["hypotheses"]) == r["iterations"] and best == r["count"] and r["skipped"] == 0
    assert r["iterations"] >= math.log(0.01) / math.log(1 - 0.8 ** 3) - 1  # no sample can do better than the ground's share
    # every ground point lies within the noise of z = -1.7; the winner holds `count` points within 0.1 of itself
    assert r["count"] >= 0.9 * len(ground)
    inl = r["inliers"]
    assert len(inl) == r["count"] and np.all(np.diff(inl) > 0)
    flat = pts[inl].copy()
    flat[:, 2] = gs.GROUND_Z
    assert np.max(np.abs(gr.plane_distance(r["coef"], flat))) < 0.1 + 0.02 + 1e-4
    assert abs(abs(float(r["coef"][2])) - 1) < 0.01


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_batched_replay_is_the_sequential_loop(batch):
    pts, _ = _known_plane(seed=5, n_in=500, n_out=500)  # a share of 0.5: k is in the thirties, several batches of 7
    a, b = gr.ransac(pts), gr.ransac_batched(pts, batch)
    assert a["iterations"] > 7
    assert (a["sample"], a["count"], a["iterations"], a["skipped"], a["k"]) == (b["sample"], b["count"], b["iterations"], b["skipped"], b["k"])
    assert a["coef"].tobytes() == b["coef"].tobytes() and np.array_equal(a["inliers"], b["inliers"])
    assert [h[0] for h in a["hypotheses"]] == [h[0] for h in b["hypotheses"]]


def test_all_coplanar_clamps_k():
    pts = gs.patch(600, noise=0.0)
    r = gr.ransac(pts)
    assert r["count"] == 600 and r["iterations"] == 1
    assert r["k"] == math.log(0.01) / math.log(gr.DBL_EPS)


def test_injected_degenerate_sample_is_skipped_not_counted():
    pts = _line_cloud()
    r = gr.ransac(pts, samples=[(3, 17, 40), (3, 17, 48)])
    assert r["skipped"] == 1 and r["iterations"] == 1 and r["sample"] == (3, 17, 48)
    assert [h[3] for h in r["hypotheses"]] == [0, 1]


def test_axis_aligned_collinear_points_pass_the_reference_test():
    """isSampleGood compares ratios: 0 / 0 is NaN and unequal to everything, so three points on a line along an axis are
    a "good" sample; their plane is NaN and holds no point.  Kept as the reference has it."""
    pts = gs.lattice()
    assert not gr.collinear(pts[0], pts[1], pts[2])
    coef = gr.plane_of(pts[0], pts[1], pts[2])
    assert np.all(np.isnan(coef)) and gr.within(coef, pts).sum() == 0


# ------------------------------------------------------------------------------------------------ clip, gates, quirks
def test_tilt_zero_is_a_bitwise_no_op():
    cloud = gs.scene(2)
    T, Ti = gr.tilt_matrix(0.0)
    assert np.array_equal(T, np.eye(4, dtype=F32)) and np.array_equal(Ti, np.eye(4, dtype=F32))
    assert gr.move(T, cloud).tobytes() == cloud.tobytes() == gr.move(Ti, cloud).tobytes()


def test_clip_edges():
    below = np.nextafter(F32(0.5), F32(0))
    z = np.array([-4.5, np.nextafter(F32(-4.5), F32(-5)), below, 0.5, 0.0, -1.7, np.nan], F32)
    cloud = np.column_stack([np.full(len(z), 3.0), np.full(len(z), -2.0), z, np.zeros(len(z))]).astype(F32)
    assert list(gr.clip_mask(cloud)) == [True, False, True, False, True, True, False]
    # the dot product as written is the z compare for every finite z when x and y are finite: (0 x + 0 y) is a zero,
    # a zero plus 1 z is z (or +0 for z = -0, which adds to d as -0 does)
    rng = np.random.default_rng(0)
    zz = rng.uniform(-6, 2, 20000).astype(F32)
    c = np.column_stack([rng.uniform(-60, 60, (20000, 2)), zz, np.zeros(20000)]).astype(F32)
    assert np.array_equal(gr.clip_mask(c), (zz >= F32(-4.5)) & (zz < F32(0.5)))


def test_reason_too_few_points_at_511():
    a, b = gr.detect(gs.patch(511)), gr.detect(gs.patch(512))
    assert (a["n_normal"], a["found"], a["reason"]) == (511, False, "TOO_FEW_POINTS") and a["iterations"] == 0
    assert (b["n_normal"], b["found"], b["reason"]) == (512, True, "OK")


def test_reason_too_few_inliers_at_511():
    a = gr.detect(gs.plane_and_clutter(511, 200), use_normal_filtering=False)
    b = gr.detect(gs.plane_and_clutter(512, 200), use_normal_filtering=False)
    assert (a["n_normal"], a["n_inliers"], a["found"], a["reason"]) == (711, 511, False, "TOO_FEW_INLIERS")
    assert (b["n_normal"], b["n_inliers"], b["found"], b["reason"]) == (712, 512, True, "OK")


def test_reason_not_vertical_past_ten_degrees_and_the_tilt_compensates():
    cloud = gs.rotate_y(gs.patch(900, extent=9.0), 12.0)
    a = gr.detect(cloud)
    assert a["n_inliers"] >= 512 and (a["found"], a["reason"]) == (False, "NOT_VERTICAL")
    b = gr.detect(cloud, tilt_deg=-12.0)
    assert b["found"] and b["reason"] == "OK"
    # the coefficients are in the input's frame: the floor's normal is 12 degrees off vertical there
    # (a plane that holds 512 points of a 18 m patch within 0.1 m is within atan(0.2 / 9) = 1.3 degrees of it)
    assert abs(math.degrees(math.acos(float(b["coeffs"][2]))) - 12.0) < 1.3
    c = gr.detect(gs.rotate_y(gs.patch(900, extent=9.0), 8.0))
    assert c["found"]


def test_downward_normal_comes_back_negated():
    cloud = gs.patch(600, noise=0.0)
    up = gr.detect(cloud, samples=[(0, 1, 2)], use_normal_filtering=False)
    down = gr.detect(cloud, samples=[(0, 2, 1)], use_normal_filtering=False)
    raw = [h[1] for h in up["hypotheses"]][0], [h[1] for h in down["hypotheses"]][0]
    assert raw[0][2] * raw[1][2] < 0  # one of the two samples gives the downward normal
    assert np.array_equal(raw[0], -raw[1])
    assert up["found"] and down["found"] and up["coeffs"][2] > 0
    assert np.array_equal(up["coeffs"], down["coeffs"])  # equal up to the sign of a zero: x - y and y - x are both +0


def test_literal_no_ground_differs_and_the_default_removes_the_inliers_origins():
    cloud = gs.scene(4)
    a, b = gr.detect(cloud), gr.detect(cloud, literal_no_ground=True)
    assert a["found"] and b["found"]
    assert not np.array_equal(a["normal_org"], np.arange(a["n_normal"]))  # filtered and input indices differ
    origins = a["normal_org"][a["inliers"]]
    keep = np.ones(len(cloud), bool)
    keep[origins] = False
    assert a["no_ground"].tobytes() == cloud[keep].tobytes() and len(a["no_ground"]) == len(cloud) - a["n_inliers"]
    assert a["ground"][:, 3].tobytes() == cloud[origins][:, 3].tobytes()  # the intensities name the points
    assert len(b["no_ground"]) == len(a["no_ground"]) and b["no_ground"].tobytes() != a["no_ground"].tobytes()
    lit = np.ones(len(cloud), bool)
    lit[b["inliers"]] = False
    assert b["no_ground"].tobytes() == cloud[lit].tobytes()


def test_scene_exercises_what_it_is_for():
    cloud = gs.scene(0)
    r = gr.detect(cloud)
    assert 3000 <= len(cloud) <= 6000
    assert r["found"] and r["n_clipped"] < len(cloud) and 512 <= r["n_normal"] < r["n_clipped"]
    assert r["n_normal"] > 256  # more than one scoring workgroup
    assert abs(float(r["coeffs"][3]) + gs.GROUND_Z) < 0.05 and r["coeffs"][2] > 0.999


def test_normal_filter_margin_excludes_under_one_percent():
    """The GPU test compares keep flags outside a margin of ten times the restatement's own spread (neighbour sums
    forwards against backwards); the chosen scene must leave under 1 % of its points inside it."""
    for cloud in (gs.scene(0), gs.lattice()):
        clipped = cloud[gr.clip_mask(cloud)]
        m = gr.keep_margin(clipped, exact=len(clipped) < 2500)
        # at most f32 roundings of the normal (the two summation orders may well round alike: a margin of zero then
        # holds the device to every point but the degenerate ones)
        assert m["margin"] < 1e-4, m["margin"]
        assert m["excluded"].mean() < 0.01, (m["margin"], m["excluded"].sum())
