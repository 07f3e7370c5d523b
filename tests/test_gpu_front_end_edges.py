"""filter_node's front end on the device at its edges: every case of front_end_cases.py (k-NN lane lists of 32 and 64,
ring exit, block shells, doubled index cell, VoxelGrid overflow copy, ties, crop boundaries) against the oracle's
brute-force reference with the bars of test_front_end.py (n_voxel equal, per-point distances bit for bit, threshold
within 1e-12, kept rows bit for bit), then the C-ABI entry points no other test compares (device-resident filter,
strided PointXYZI records, a small cap, parameter rejection), pcl::VoxelGrid and pcl::transformPointCloud on their own.
test_front_end_cases.py (CPU) shows that every case is well posed and that the reference follows PCL's definition."""
import ctypes as C

import numpy as np
import pytest

from front_end_cases import CASE_IDS, CASES, bits, cloud_of, crop_edges, lattice, reference, scattered
from helpers import f32_transform

pytestmark = pytest.mark.gpu

xa = pytest.importorskip("xchu_slam_amd")
from xchu_slam_amd import _lib  # noqa: E402

SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def ndt():
    g = xa.NormalDistributionsTransform()
    yield g
    g.close()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _params(ndt, **kw):
    prm = _lib.FilterParams()
    assert ndt._lib.ndt_filter_default_params(C.byref(prm)) == _lib.NDT_OK
    for k, v in kw.items():
        setattr(prm, k, v)
    return prm


def _stats(ndt, n):
    dist = np.zeros(max(1, n), np.float32)
    nv = C.c_size_t()
    thr = np.zeros(3, np.float64)
    assert ndt._lib.ndt_filter_last_stats(ndt.ctx, _fp(dist), n, C.byref(nv), thr.ctypes.data_as(C.POINTER(C.c_double))) == _lib.NDT_OK
    return dist[: nv.value].copy(), thr, nv.value


def _filter_host(ndt, rows, prm, intensity_offset=3, cap=None, stride_bytes=None):
    """ndt_filter_scan on host rows of any width: (status, caller's buffer, n_out)."""
    rows = np.ascontiguousarray(rows, np.float32)
    n = len(rows)
    out = np.full((max(1, n), 4), SENTINEL, np.float32)
    nout = C.c_size_t()
    st = ndt._lib.ndt_filter_scan(ndt.ctx, C.byref(prm), _fp(rows), n, rows.shape[1] * 4 if stride_bytes is None else stride_bytes,
                                  intensity_offset, _fp(out), n if cap is None else cap, C.byref(nout))
    return st, out, nout.value


def _download(ndt, ptr, n):
    out = np.empty((max(1, n), 4), np.float32)
    assert ndt._lib.ndt_synchronize(ndt.ctx) == _lib.NDT_OK
    assert ndt._lib.ndt_memcpy_d2h(ndt.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), n * 16) == _lib.NDT_OK
    return out[:n]


def _wide(cloud):
    """(N, 8) records with pcl::PointXYZI's layout: x, y, z, padding, intensity, padding; the padding poisoned."""
    w = np.full((len(cloud), 8), np.nan, np.float32)
    w[:, :3] = cloud[:, :3]
    w[:, 4] = cloud[:, 3]
    return w


SOR_RUN = dict(leaf=0.3)
ROR_RUN = dict(outlier_method=1, ror_radius=0.8, ror_min_neighbors=5)


# ---------------------------------------------------------------- every case against the brute-force reference
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_filter_scan_case(oracle, ndt, case):
    cloud = cloud_of(case)
    od, odist, othr, onv = reference(oracle, case)
    gd, gdist, gthr, gnv = xa.filter_scan(cloud, stats=True, ndt=ndt, **case.kw)
    assert gnv == onv
    if case.kw.get("outlier_method", 0) == 0 and onv > case.kw.get("mean_k", 30):
        bad = np.flatnonzero(gdist != odist)
        assert len(bad) == 0, (len(bad), bad[:8], gdist[bad[:8]], odist[bad[:8]])
        assert abs(gthr[0] - othr[0]) <= 1e-12 * abs(othr[0])
    assert gd.shape == od.shape and np.array_equal(bits(gd), bits(od))


# ---------------------------------------------------------------- C-ABI entry points
@pytest.mark.parametrize("gen", [scattered, crop_edges], ids=["scattered", "crop_edges"])
@pytest.mark.parametrize("run", [SOR_RUN, ROR_RUN], ids=["sor", "ror"])
def test_filter_scan_device_equals_host(ndt, gen, run):
    """ndt_filter_scan_device (device float4 in and out) against ndt_filter_scan: same rows, count and statistics."""
    cloud = np.ascontiguousarray(gen(), np.float32)
    n = len(cloud)
    prm = _params(ndt, **run)
    st, hout, hn = _filter_host(ndt, cloud, prm)
    assert st == _lib.NDT_OK and hn < n and (hn > 0 or gen is crop_edges)
    hdist, hthr, hnv = _stats(ndt, n)
    d_in = ndt.device_upload(cloud)
    d_out = ndt.device_upload(np.full((n, 4), SENTINEL, np.float32))
    try:
        nout = C.c_size_t()
        assert ndt._lib.ndt_filter_scan_device(ndt.ctx, C.byref(prm), C.c_void_p(d_in), n, C.c_void_p(d_out), C.byref(nout)) == _lib.NDT_OK
        assert nout.value == hn
        assert np.array_equal(bits(_download(ndt, d_out, n)[:hn]), bits(hout[:hn]))
        assert np.array_equal(bits(_download(ndt, d_in, n)), bits(cloud))  # the input is left as it was
        ddist, dthr, dnv = _stats(ndt, n)
        assert dnv == hnv
        if run is SOR_RUN and hnv > prm.mean_k:
            assert np.array_equal(ddist, hdist) and np.array_equal(dthr, hthr)
        assert ndt._lib.ndt_filter_scan_device(ndt.ctx, C.byref(prm), C.c_void_p(d_in), n, C.c_void_p(d_in), C.byref(nout)) == _lib.NDT_EINVAL
    finally:
        ndt.device_free(d_in)
        ndt.device_free(d_out)


@pytest.mark.parametrize("gen", [scattered, crop_edges], ids=["scattered", "crop_edges"])
@pytest.mark.parametrize("run", [SOR_RUN, ROR_RUN], ids=["sor", "ror"])
def test_filter_scan_strided_records(ndt, gen, run):
    """stride_bytes = 32, intensity_offset = 4 (pcl::PointXYZI as an integrating host passes it) equals the packed call."""
    cloud = np.ascontiguousarray(gen(), np.float32)
    prm = _params(ndt, **run)
    st, pout, pn = _filter_host(ndt, cloud, prm)
    assert st == _lib.NDT_OK and (pn > 0 or gen is crop_edges)
    st, wout, wn = _filter_host(ndt, _wide(cloud), prm, intensity_offset=4)
    assert st == _lib.NDT_OK and wn == pn
    assert np.array_equal(bits(wout), bits(pout))


def test_filter_scan_bad_layout(ndt):
    cloud = np.ascontiguousarray(scattered()[:64], np.float32)
    prm = _params(ndt)
    wide = _wide(cloud)
    assert _filter_host(ndt, wide, prm, intensity_offset=2)[0] == _lib.NDT_EINVAL
    assert _filter_host(ndt, wide, prm, intensity_offset=3, stride_bytes=12)[0] == _lib.NDT_EINVAL
    assert _filter_host(ndt, wide, prm, intensity_offset=8)[0] == _lib.NDT_EINVAL   # 8 * 4 + 4 > 32
    assert _filter_host(ndt, cloud, prm, intensity_offset=4)[0] == _lib.NDT_EINVAL  # 4 * 4 + 4 > 16
    out = np.zeros((64, 4), np.float32)
    nout = C.c_size_t()
    for ioff, stride in ((2, 32), (3, 12), (8, 32)):
        assert ndt._lib.ndt_voxel_downsample(ndt.ctx, _fp(wide), 64, stride, ioff, 0.5, _fp(out), 64, C.byref(nout)) == _lib.NDT_EINVAL


@pytest.mark.parametrize("run", [SOR_RUN, ROR_RUN], ids=["sor", "ror"])
def test_filter_scan_small_cap(ndt, run):
    """cap below the output: *n_out reports the full count, cap rows are written, the caller's rows after them are not."""
    cloud = np.ascontiguousarray(scattered(), np.float32)
    prm = _params(ndt, **run)
    st, full, n_full = _filter_host(ndt, cloud, prm)
    assert st == _lib.NDT_OK and n_full >= 2
    cap = n_full // 2
    st, part, n_part = _filter_host(ndt, cloud, prm, cap=cap)
    assert st == _lib.NDT_OK and n_part == n_full
    assert np.array_equal(bits(part[:cap]), bits(full[:cap]))
    assert np.all(part[cap:] == SENTINEL)


@pytest.mark.parametrize("bad", [dict(mean_k=0), dict(mean_k=64), dict(r_min=60.0, r_max=60.0), dict(r_min=61.0), dict(outlier_method=2),
                                 dict(outlier_method=-1), dict(outlier_method=1, ror_radius=0.0), dict(leaf=0.0),
                                 dict(leaf=float("nan"))], ids=str)
def test_filter_scan_rejects_parameters(ndt, bad):
    cloud = np.ascontiguousarray(scattered()[:64], np.float32)
    st, out, n_out = _filter_host(ndt, cloud, _params(ndt, **bad))
    assert st == _lib.NDT_EINVAL and n_out == 0
    assert np.all(out == SENTINEL)


# ---------------------------------------------------------------- pcl::VoxelGrid on its own
def _one_voxel():
    """5000 points inside one 2 m voxel: the float sum runs over them in input order."""
    rng = np.random.default_rng(120)
    p = rng.uniform([4.0, 6.0, 0.0], [6.0, 8.0, 2.0], (5000, 3))
    return np.concatenate([p, rng.uniform(0, 1, (5000, 1))], 1).astype(np.float32), 2.0


def _negative():
    rng = np.random.default_rng(121)
    p = rng.uniform([-50.0, -40.0, -9.0], [-20.0, -10.0, -1.0], (3000, 3))
    return np.concatenate([p, rng.uniform(0, 1, (3000, 1))], 1).astype(np.float32), 0.5


VOXEL_CASES = {
    "scattered-0.1": lambda: (scattered(), 0.1), "scattered-0.3": lambda: (scattered(), 0.3),
    "scattered-0.5": lambda: (scattered(), 0.5), "scattered-2.0": lambda: (scattered(), 2.0),
    "one-voxel": _one_voxel, "n1": lambda: (scattered()[:1], 0.5), "negative": _negative,
    # every point on a voxel face (0.75 = 1 * 0.75 = 3 * 0.25)
    "lattice-0.75": lambda: (lattice(), 0.75), "lattice-0.25": lambda: (lattice(), 0.25),
    # 60 m / 1e-4 = 6e5 voxels per axis: far more than 2^31 in all, pcl::VoxelGrid returns the input
    "overflow": lambda: (scattered()[:2000], 1e-4),
}


@pytest.mark.parametrize("name", list(VOXEL_CASES))
def test_voxel_downsample_host_and_device(oracle, ndt, name):
    """ndt_voxel_downsample (packed and PointXYZI records) and ndt_voxel_downsample_device against the oracle, bit for
    bit; on overflow NDT_EOVERFLOW and the input in input order."""
    cloud, leaf = VOXEL_CASES[name]()
    cloud = np.ascontiguousarray(cloud, np.float32)
    n = len(cloud)
    ref = oracle.voxel_downsample(cloud, leaf)
    overflow = name == "overflow"
    if overflow:
        assert np.array_equal(ref, cloud)
    elif name == "one-voxel":
        assert len(ref) == 1
    want = _lib.NDT_EOVERFLOW if overflow else _lib.NDT_OK
    for rows, ioff in ((cloud, 3), (_wide(cloud), 4)):
        out = np.full((n, 4), SENTINEL, np.float32)
        nout = C.c_size_t()
        st = ndt._lib.ndt_voxel_downsample(ndt.ctx, _fp(rows), n, rows.shape[1] * 4, ioff, leaf, _fp(out), n, C.byref(nout))
        assert st == want and nout.value == len(ref)
        assert np.array_equal(bits(out[: len(ref)]), bits(ref))
        assert np.all(out[len(ref):] == SENTINEL)
    assert np.array_equal(bits(xa.voxel_downsample(cloud, leaf, ndt=ndt)), bits(ref))
    d_in = ndt.device_upload(cloud)
    d_out = ndt.device_upload(np.full((n, 4), SENTINEL, np.float32))
    try:
        nout = C.c_size_t()
        st = ndt._lib.ndt_voxel_downsample_device(ndt.ctx, C.c_void_p(d_in), n, leaf, C.c_void_p(d_out), C.byref(nout))
        assert st == want and nout.value == len(ref)
        assert np.array_equal(bits(_download(ndt, d_out, n)[: len(ref)]), bits(ref))
        assert np.array_equal(bits(_download(ndt, d_in, n)), bits(cloud))
    finally:
        ndt.device_free(d_in)
        ndt.device_free(d_out)


def test_voxel_downsample_small_cap(oracle, ndt):
    cloud = np.ascontiguousarray(scattered(), np.float32)
    ref = oracle.voxel_downsample(cloud, 0.5)
    cap = len(ref) // 2
    out = np.full((len(cloud), 4), SENTINEL, np.float32)
    nout = C.c_size_t()
    assert ndt._lib.ndt_voxel_downsample(ndt.ctx, _fp(cloud), len(cloud), 16, 3, 0.5, _fp(out), cap, C.byref(nout)) == _lib.NDT_OK
    assert nout.value == len(ref)
    assert np.array_equal(bits(out[:cap]), bits(ref[:cap])) and np.all(out[cap:] == SENTINEL)


# ---------------------------------------------------------------- pcl::transformPointCloud on device clouds
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_transform_device(ndt, n):
    """Out of place and in place against the float32 restatement, bit for bit; the intensity carried through, the
    rows after n untouched."""
    rng = np.random.default_rng(130 + n)
    cloud = np.concatenate([rng.uniform(-60, 60, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    cloud[0, 3] = np.nan
    T = np.array(xa.synth.pose_matrix(3.0, -2.0, 0.5, 0.02, -0.03, 0.7), np.float32)
    ref = np.concatenate([f32_transform(T, cloud), cloud[:, 3:]], 1)
    Tc = np.ascontiguousarray(T.T).reshape(-1)
    tail = np.full((3, 4), SENTINEL, np.float32)
    d_in = ndt.device_upload(np.concatenate([cloud, tail]))
    d_out = ndt.device_upload(np.full((n + 3, 4), SENTINEL, np.float32))
    try:
        assert ndt._lib.ndt_transform_device(ndt.ctx, _fp(Tc), C.c_void_p(d_in), n, C.c_void_p(d_out)) == _lib.NDT_OK
        got = _download(ndt, d_out, n + 3)
        assert np.array_equal(bits(got[:n]), bits(ref)) and np.all(got[n:] == SENTINEL)
        assert np.array_equal(bits(_download(ndt, d_in, n)), bits(cloud))
        assert ndt._lib.ndt_transform_device(ndt.ctx, _fp(Tc), C.c_void_p(d_in), n, C.c_void_p(d_in)) == _lib.NDT_OK
        got = _download(ndt, d_in, n + 3)
        assert np.array_equal(bits(got[:n]), bits(ref)) and np.all(got[n:] == SENTINEL)
    finally:
        ndt.device_free(d_in)
        ndt.device_free(d_out)
