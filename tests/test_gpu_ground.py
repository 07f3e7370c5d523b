"""filter_node's ground detection on the device against its restatement (tests/ground_restate.py): origin indices and
neighbours exact, keep flags exact outside the measured margin, every hypothesis' count exact and its coefficients bit for
bit, and with the device's own sampler the same samples, hence the same floor and clouds."""
import ctypes as C

import numpy as np
import pytest

import ground_restate as gr
import ground_scene as gs

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def xa():
    import xchu_slam_amd
    return xchu_slam_amd


@pytest.fixture(scope="module")
def cf(xa):
    f = xa.CloudFilter(cloud_leaf=0.0)
    yield f
    f.close()


def _defaults(cf):
    cf.set_samples(None)
    cf.set_params(cloud_leaf=0.0, **gr.DEFAULTS)


_REF = {}


def _reference(name, cloud, **params):
    """The restatement of a scene, computed once and shared."""
    key = (name, tuple(sorted(params.items())))
    if key not in _REF:
        _REF[key] = gr.detect(cloud, **params)
    return _REF[key]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(cf, name, cloud, **params):
    """One detect on the device against the restatement: record, winner, coefficients bit for bit, raw clouds bit for bit."""
    _defaults(cf)
    cf.set_params(**params)
    ref = _reference(name, cloud, **params)
    dev = cf.detect_plane(cloud)
    got = (dev.n_input, dev.n_clipped, dev.n_normal, dev.found, dev.reason, dev.iterations, dev.skipped, dev.winner, dev.n_inliers)
    want = (ref["n_input"], ref["n_clipped"], ref["n_normal"], ref["found"], ref["reason"], ref["iterations"], ref["skipped"],
            ref["winner"], ref["n_inliers"])
    print(name, "device", got, "k", dev.k, "restated k", ref["k"])
    assert got == want
    assert dev.stream_fallbacks == 0
    if ref["iterations"]:
        assert abs(dev.k - ref["k"]) <= 1e-12 * abs(ref["k"])  # the two libraries' log may round apart
    if ref["found"]:
        assert _same_bits(dev.coeffs, ref["coeffs"])
    else:
        assert dev.coeffs is None
    for cloud_name in ("normal_ground", "ground", "no_ground"):
        assert _same_bits(getattr(dev, cloud_name)(), ref[cloud_name]), cloud_name
    return dev, ref


# ------------------------------------------------------------------------------------------------ clip and normals
@pytest.mark.parametrize("name", ["scene", "lattice"])
def test_origin_indices_neighbours_and_keep_flags(cf, name):
    cloud = gs.scene(0) if name == "scene" else gs.lattice()
    _defaults(cf)
    cf.detect_plane(cloud)
    nrm4, keep, org, nbr = cf.last_normals()
    clip_org = np.flatnonzero(gr.clip_mask(cloud))
    assert np.array_equal(org, clip_org) and 0 < len(clip_org) < len(cloud)
    # the lattice through every pair's f32 distance: exact under any number of ties
    m = gr.keep_margin(cloud[clip_org], exact=name == "lattice")
    assert np.array_equal(nbr, m["fwd"]["nn"])
    if name == "lattice":  # deliberate ties: most points have several neighbours at one distance
        d2 = gr.knn_bruteforce(cloud[clip_org][:, :3], 10)[1]
        assert (np.diff(d2, axis=1) == 0).any(axis=1).mean() > 0.9
    excluded = m["excluded"]
    print(name, "margin", m["margin"], "excluded", int(excluded.sum()), "of", len(excluded),
          "max |n.z| difference", float(np.nanmax(np.abs(nrm4[:, 3] - m["fwd"]["absz"]))))
    assert excluded.mean() <= 0.01
    assert np.array_equal(keep[~excluded].astype(bool), m["keep"][~excluded])
    # the normals point to the viewpoint (0, 0, sensor_height)
    v = np.array([0, 0, 2.0]) - cloud[clip_org][:, :3].astype(np.float64)
    assert np.all(np.einsum("ij,ij->i", v, nrm4[:, :3].astype(np.float64)) >= -1e-5)


# ------------------------------------------------------------------------------------------------ RANSAC, injected samples
def test_injected_samples_counts_coefficients_and_winner(cf):
    cloud = gs.scene(0)
    ref0 = _reference("scene", cloud)
    filtered = ref0["normal_ground"]
    s = gr.Sampler(filtered, seed=777)  # another stream than the device's own
    triples = [s.sample() for _ in range(70)]
    triples[5] = (triples[5][0], triples[5][0], triples[5][1])  # a repeated point: all ratios 0, a degenerate sample
    ref = gr.detect(cloud, samples=triples)
    _defaults(cf)
    cf.set_samples(triples)
    try:
        dev = cf.detect_plane(cloud)
        tri, coef, cnt, stat = cf.last_hypotheses()
        ground = dev.ground()
    finally:
        cf.set_samples(None)
    assert dev.n_normal == ref["n_normal"]
    hyp = ref["hypotheses"]
    assert len(tri) == len(hyp) and [tuple(t) for t in tri.tolist()] == [h[0] for h in hyp]
    assert cnt.tolist() == [h[2] for h in hyp] and stat.tolist() == [h[3] for h in hyp]
    for c, h in zip(coef, hyp):
        assert np.all(np.isnan(c)) if h[1] is None or np.all(np.isnan(h[1])) else _same_bits(c, h[1])
    assert (dev.iterations, dev.skipped, dev.winner, dev.n_inliers) == (ref["iterations"], ref["skipped"], ref["winner"], ref["n_inliers"])
    assert _same_bits(dev.coeffs, ref["coeffs"]) and _same_bits(ground, ref["ground"])  # the inlier list, in index order


def test_injected_degenerate_sample_is_skipped(cf):
    i = np.arange(600, dtype=np.float64)
    line = np.column_stack([i * 0.01, i * 0.02, -1.7 + i * 0.001, np.zeros(600)]).astype(F32)
    cloud = np.concatenate([line, gs.patch(600, noise=0.0)])
    triples = [(8, 16, 32), (600, 700, 900)]  # the first three lie on the line exactly: equal ratios
    assert gr.collinear(cloud[8], cloud[16], cloud[32])
    ref = gr.detect(cloud, samples=triples, use_normal_filtering=False)
    _defaults(cf)
    cf.set_params(use_normal_filtering=0)
    cf.set_samples(triples)
    try:
        dev = cf.detect_plane(cloud)
        stat = cf.last_hypotheses()[3]
    finally:
        cf.set_samples(None)
    assert ref["skipped"] == 1 and (dev.skipped, dev.iterations, dev.found) == (ref["skipped"], ref["iterations"], ref["found"])
    assert stat.tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_with_the_device_sampler(cf, xa):
    cloud = gs.scene(0)
    dev, ref = _compare(cf, "scene", cloud)
    assert dev.found and len(cloud) % 256 != 0 and dev.n_normal % 256 != 0
    tri = cf.last_hypotheses()[0]
    assert [tuple(t) for t in tri.tolist()] == [h[0] for h in ref["hypotheses"]]  # the same samples
    # run to run
    again = cf.detect_plane(cloud)
    assert _same_bits(again.coeffs, dev.coeffs) and again.winner == dev.winner and again.iterations == dev.iterations
    for cloud_name in ("normal_ground", "ground", "no_ground"):
        assert _same_bits(getattr(again, cloud_name)(), getattr(dev, cloud_name)())
    # the clouds through the 0.2 m VoxelGrid: the library's own downsample of the restated raw clouds
    cf.set_params(cloud_leaf=0.2)
    leafed = cf.detect_plane(cloud)
    for cloud_name in ("normal_ground", "ground", "no_ground"):
        got = getattr(leafed, cloud_name)()
        want = xa.voxel_downsample(ref[cloud_name], 0.2, ndt=cf.registration)
        assert 0 < len(got) <= len(ref[cloud_name]) and _same_bits(got, want), cloud_name
    _defaults(cf)


def test_detect_strided_records(cf, xa):
    """ndt_ground_detect over 32-byte records with the intensity at float 4 (pcl::PointXYZI's layout, the padding
    poisoned): the result record and the three clouds of the packed (N, 4) call."""
    from xchu_slam_amd import ground
    cloud = np.ascontiguousarray(gs.scene(0), F32)
    wide = np.full((len(cloud), 8), np.nan, F32)
    wide[:, :3] = cloud[:, :3]
    wide[:, 4] = cloud[:, 3]
    _defaults(cf)
    packed = cf.detect_plane(cloud)
    clouds = [getattr(packed, name)() for name in ("normal_ground", "ground", "no_ground")]
    assert packed.found and all(len(c) > 0 for c in clouds)
    rec = ground._record()
    st = cf._lib.ndt_ground_detect(cf.ctx, C.byref(cf._gprm), wide.ctypes.data_as(C.POINTER(C.c_float)), len(wide), 32, 4, C.byref(rec))
    assert st == 0
    strided = ground.GroundResult(cf.registration, rec)
    fields = ("found", "reason", "n_input", "n_clipped", "n_normal", "n_inliers", "iterations", "skipped", "k", "winner", "stream_fallbacks")
    assert [getattr(strided, f) for f in fields] == [getattr(packed, f) for f in fields]
    assert _same_bits(strided.coeffs, packed.coeffs)
    for name, want in zip(("normal_ground", "ground", "no_ground"), clouds):
        assert _same_bits(getattr(strided, name)(), want), name


def test_literal_no_ground(cf):
    cloud = gs.scene(4)
    dev, ref = _compare(cf, "scene4-literal", cloud, literal_no_ground=True)
    plain, _ = _compare(cf, "scene4", cloud)
    assert dev.found and not _same_bits(dev.no_ground(), plain.no_ground())


EDGES = {
    "empty": (lambda: np.zeros((0, 4), F32), {}),
    "two_after_clip": (lambda: np.concatenate([gs.patch(2), gs.patch(60, z=1.5)]), {}),
    "seven_after_clip": (lambda: np.concatenate([gs.patch(7), gs.patch(60, z=1.5)]), {}),
    "511_after_normal_filter": (lambda: gs.patch(511), {}),
    "512_after_normal_filter": (lambda: gs.patch(512), {}),
    "511_inliers": (lambda: gs.plane_and_clutter(511, 200), dict(use_normal_filtering=False)),
    "512_inliers": (lambda: gs.plane_and_clutter(512, 200), dict(use_normal_filtering=False)),
    "all_coplanar": (lambda: gs.patch(600, noise=0.0), {}),
    "no_normal_filtering": (lambda: gs.scene(2), dict(use_normal_filtering=False)),
    "tilt_5": (lambda: gs.rotate_y(gs.scene(3), 5.0), dict(tilt_deg=-5.0)),
    "not_vertical": (lambda: gs.rotate_y(gs.patch(900, extent=9.0), 12.0), {}),
    "second_batch": (lambda: gs.scene(5, radius=11.0, clutter=2500, walls=False), dict(use_normal_filtering=False)),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(cf, name):
    make, params = EDGES[name]
    cloud = make()
    dev, ref = _compare(cf, name, cloud, **params)
    if name == "empty":
        assert (dev.n_input, dev.reason) == (0, "TOO_FEW_POINTS")
    if name in ("two_after_clip", "seven_after_clip"):
        nrm4, keep, org, nbr = cf.last_normals()
        assert len(keep) == dev.n_clipped == int(name.startswith("two")) * 2 + int(name.startswith("seven")) * 7
        assert keep.astype(bool).tolist() == ref["keep"].tolist()  # two points: NaN normals, none kept; seven: all of them
        assert np.array_equal(nbr[:, : dev.n_clipped], ref["normals"]["nn"]) and np.all(nbr[:, dev.n_clipped:] == -1)
    if name == "all_coplanar":
        assert dev.n_inliers == dev.n_normal == 600 and dev.iterations == 1
    if name == "tilt_5":
        assert dev.found and abs(np.degrees(np.arccos(float(dev.coeffs[2]))) - 5.0) < 1.3
    if name == "not_vertical":
        assert dev.reason == "NOT_VERTICAL" and dev.n_inliers >= 512
    if name == "second_batch":
        assert dev.iterations > cf.batch and ref["k"] > cf.batch  # the fit needed a later batch (and here a later chain)
    if name.endswith("_inliers"):
        assert dev.reason == ("OK" if name.startswith("512") else "TOO_FEW_INLIERS")
    if name.endswith("after_normal_filter"):
        assert dev.reason == ("OK" if name.startswith("512") else "TOO_FEW_POINTS")


def test_a_scan_past_the_generator_table_is_continued_and_counted(xa, monkeypatch):
    """A context whose first table holds 32 words: the 114 iterations of the low-share scene draw 342, so the host
    continues the stream four times (64, 128, 256, 512 words), and the floor is the one of the full table."""
    make, params = EDGES["second_batch"]
    cloud = make()
    ref = _reference("second_batch", cloud, **params)
    monkeypatch.setenv("NDT_GROUND_STREAM", "32")
    short = xa.CloudFilter(cloud_leaf=0.0, use_normal_filtering=0)
    try:
        dev = short.detect_plane(cloud)
        assert dev.stream_fallbacks == 4
        assert (dev.found, dev.iterations, dev.winner, dev.n_inliers) == (ref["found"], ref["iterations"], ref["winner"], ref["n_inliers"])
        assert _same_bits(dev.coeffs, ref["coeffs"]) and _same_bits(dev.ground(), ref["ground"])
        again = short.detect_plane(cloud)  # the longer table stays with the context
        assert again.stream_fallbacks == 0 and _same_bits(again.coeffs, ref["coeffs"])
    finally:
        short.close()


# ------------------------------------------------------------------------------------------------ the node's Run
def test_filter_ground_scan_is_filter_scan_then_detect(cf, xa):
    rng = np.random.default_rng(11)
    base = gs.scene(6)
    # a raw scan: several returns per 0.5 m voxel, some stray points and non-finite ones
    raw = np.repeat(base, 3, axis=0)
    raw[:, :3] += rng.normal(0, 0.04, (len(raw), 3)).astype(F32)
    raw[::97, 2] += 6.0
    raw[5, 0] = np.nan
    _defaults(cf)
    filtered, floor = cf.run(raw)
    want = xa.filter_scan(raw, ndt=cf.registration)
    assert _same_bits(filtered, want) and len(filtered) > 1000
    sep = cf.detect_plane(want)
    assert (floor.found, floor.reason, floor.iterations, floor.winner, floor.n_normal) == (sep.found, sep.reason, sep.iterations, sep.winner, sep.n_normal)
    assert floor.found and _same_bits(floor.coeffs, sep.coeffs)
    alone = xa.detect_ground(want, cloud_leaf=0.0)  # on a context of its own
    assert _same_bits(alone.coeffs, sep.coeffs)
    for cloud_name in ("normal_ground", "ground", "no_ground"):
        assert _same_bits(getattr(sep, cloud_name)(), getattr(alone, cloud_name)()), cloud_name


# ------------------------------------------------------------------------------------------------ life cycle
def test_two_contexts_changing_sizes_and_close(xa):
    from xchu_slam_amd import _lib
    a, b = xa.CloudFilter(cloud_leaf=0.0), xa.CloudFilter(cloud_leaf=0.0)
    try:
        big, small = gs.scene(0), gs.scene(7, radius=12.0)
        ra = a.detect_plane(big)
        rb = b.detect_plane(small)
        ra2 = a.detect_plane(small)  # smaller, then larger again: the buffers are reused or grown
        ra3 = a.detect_plane(big)
        assert _same_bits(ra3.coeffs, ra.coeffs) and _same_bits(ra2.coeffs, rb.coeffs)
        assert _same_bits(ra3.ground(), _reference("scene", big)["ground"])
        assert _same_bits(rb.ground(), _reference("scene7", small)["ground"])
        # a result's clouds are those of its context's last detect; a wrong struct size is refused with the ctx's error set
        rec = _lib.GroundResult()
        rec.struct_size = 4
        st = a._lib.ndt_ground_detect(a.ctx, None, None, 0, 16, 3, C.byref(rec))
        assert st == _lib.NDT_EINVAL and b"struct_size" in a._lib.ndt_last_error(a.ctx)
    finally:
        b.close()
    with pytest.raises(Exception):
        b.detect_plane(gs.scene(0))  # detect after close is refused
    c = xa.CloudFilter()
    n = C.c_size_t()
    assert c._lib.ndt_ground_cloud(c.ctx, 0, None, 0, C.byref(n)) == _lib.NDT_EINVAL  # no detect yet
    c.close()
    a.close()
