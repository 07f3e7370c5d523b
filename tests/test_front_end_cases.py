"""The front-end edge cases (front_end_cases.py) on the CPU: the oracle's brute-force reference against a second,
independent numpy statement of the same PCL definition, the oracle's hash-grid search against brute force where it
finishes, and the conditions that make every case well posed, so that a device mismatch on one of them is never an
ill-defined input.

The numpy restatement: removeNaNFromPointCloud + the range crop as a mask, oracle.voxel_downsample, then for
StatisticalOutlierRemoval the full float32 L2_Simple squared-distance matrix (((dx dx) + dy dy) + dz dz, the oracle's
and FLANN's operation order), the k + 1 smallest of every row in ascending order, distance = float32(sum of
sqrt(float64(d[1..k])) in ascending order / k), the sequential f64 mean / variance (the square taken in float32), keep
distance <= threshold; for RadiusOutlierRemoval the count of d < float32(radius^2) in the same matrix."""
import numpy as np
import pytest

from front_end_cases import CASE_IDS, CASES, CROP_EDGES_KEPT, bits, cloud_of, reference


def _crop(cloud, r_min=1.0, r_max=60.0, **_):
    fin = np.isfinite(cloud[:, :3]).all(1)
    x, y = cloud[:, 0].astype(np.float64), cloud[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(x * x + y * y)
        return cloud[fin & (r_min < r) & (r < r_max)]


def _sq_rows(p, lo, hi):
    """float32 squared distances from points lo..hi to all points."""
    u = p[lo:hi, None, :] - p[None, :, :]
    return (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]


def _seq_sum(a):
    """Sum along the last axis in index order (np.sum adds pairwise)."""
    return np.cumsum(a, axis=-1)[..., -1]


def restate(oracle, cloud, leaf=0.5, mean_k=30, stddev_mul=1.0, outlier_method=0, ror_radius=0.8, ror_min_neighbors=5, **kw):
    ds = oracle.voxel_downsample(_crop(cloud, **kw), leaf)
    p = np.ascontiguousarray(ds[:, :3])
    nv = len(p)
    assert p.dtype == np.float32
    if outlier_method == 1:
        r2 = np.float32(ror_radius * ror_radius)
        cnt = np.concatenate([(_sq_rows(p, lo, min(lo + 512, nv)) < r2).sum(1) for lo in range(0, nv, 512)])
        return ds[cnt >= ror_min_neighbors], None, None, nv
    if nv <= mean_k:
        return ds, None, None, nv
    # the k + 1 smallest of a row, ascending, are the head of the sorted row (partition first: same values, less work)
    near = np.concatenate([np.sort(np.partition(_sq_rows(p, lo, min(lo + 512, nv)), mean_k, axis=1)[:, :mean_k + 1], axis=1)
                           for lo in range(0, nv, 512)])
    assert near.dtype == np.float32
    dist = (_seq_sum(np.sqrt(near[:, 1:].astype(np.float64))) / mean_k).astype(np.float32)
    s = _seq_sum(dist.astype(np.float64))
    sq = _seq_sum((dist * dist).astype(np.float64))
    mean = s / float(nv)
    with np.errstate(invalid="ignore"):
        std = np.sqrt((sq - s * s / float(nv)) / (float(nv) - 1))
    thr = mean + stddev_mul * std
    return ds[~(dist.astype(np.float64) > thr)], dist, thr, nv


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reference_matches_numpy_restatement(oracle, case):
    cloud = cloud_of(case)
    out, dist, thr, nv = reference(oracle, case)
    rout, rdist, rthr, rnv = restate(oracle, cloud, **case.kw)
    assert nv == rnv
    if rdist is not None:
        assert np.array_equal(dist, rdist)
        assert thr[0] == rthr
    assert out.shape == rout.shape and np.array_equal(bits(out), bits(rout))


@pytest.mark.parametrize("case", [c for c in CASES if c.grid_ok], ids=[c.id for c in CASES if c.grid_ok])
def test_oracle_grid_search_matches_brute(oracle, case):
    """The oracle's hash-grid ring search against its brute force.  The ring loop is cubic in the ring count and does
    not finish in reasonable time on clusters, offset, overflow_dups and the small leaves (neighbours hundreds of
    cells away); those cases have the numpy restatement as their second opinion, and the oracle stays as it is."""
    out, dist, thr, nv = reference(oracle, case)
    og, dg, tg, nvg = oracle.filter_scan(cloud_of(case), brute=False, is_dense=False, **case.kw)
    assert nvg == nv
    assert np.array_equal(dg, dist)
    assert tg[0] == thr[0]
    assert np.array_equal(bits(og), bits(out))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_is_well_posed(oracle, case):
    out, dist, thr, nv = reference(oracle, case)
    sor = case.kw.get("outlier_method", 0) == 0 and nv > case.kw.get("mean_k", 30)
    assert 0 < nv <= 6000
    if sor:
        assert len(dist) == nv and np.isfinite(thr).all()
        # no distance so close to the threshold that the f64 summation order of the statistics could decide it
        gap = np.min(np.abs(dist.astype(np.float64) - thr[0])) / abs(thr[0])
        assert gap > 1e-9, gap
    if case.keeps == "some":
        assert 1 <= len(out) < nv
    else:
        assert len(out) == (nv if case.keeps == "all" else 0)


def test_known_counts(oracle):
    by_id = {c.id: c for c in CASES}
    out, _, _, nv = reference(oracle, by_id["lattice-ror0.8-5"])
    assert (nv, len(out)) == (4060, 4052)
    # VoxelGrid overflow: the crop copy, duplicates included, reaches the outlier stage
    c = by_id["overflow_dups-sor30"]
    assert reference(oracle, c)[3] == len(_crop(cloud_of(c), **c.kw)) > 1700
    c = by_id["scattered-leaf0.02"]
    assert reference(oracle, c)[3] == len(_crop(cloud_of(c), **c.kw))
    c = by_id["scattered-leaf0.03"]
    assert reference(oracle, c)[3] < len(_crop(cloud_of(c), **c.kw))
    # the five rows of crop_edges that survive, in VoxelGrid's order (ascending voxel index)
    c = by_id["crop_edges"]
    out, _, _, nv = reference(oracle, c)
    kept = cloud_of(c)[CROP_EDGES_KEPT]
    assert nv == 5 and len(out) == 5
    key = lambda a: sorted(map(tuple, bits(a).tolist()))
    want = kept.copy()
    want[want[:, 0] == 0, 0] = 0.0  # a voxel mean is 0 + x: -0.0 comes out as +0.0
    assert key(out) == key(want)
