"""The radix pass (k_radix_onesweep) at the tile counts and digit shapes where its ranking and its look-back change
path, through the public API only: targets are built from points placed around chosen cell centres (resolution 1, so a
point's cell is the integer part of its coordinates and every key digit is the test's choice) and the grid is compared
with the CPU oracle's, bit for bit: keys, counts, means, inverse covariances and centroids of the KD cloud (leaves of at
least 6 points).  The means are f64 sums in input order and every point carries its own offset inside its cell, so an
unstable sort changes them.

* Tile counts around the group boundaries of the two-level look-back (groups of 16 tiles, 1024-key tiles): point counts
  of 1, 2, 16, 17, 256, 257 and 1024 times 1024, and each plus one.  The sort takes 1024-key tiles while it has fewer
  4096-key tiles than the device has CUs: on the 256 CUs of an MI355X the last two counts are 256 and 257 tiles of 4096.
* Digit shapes of the ranking: one voxel for every point (the 64 lanes of every item share a digit); 64 consecutive
  points in 64 different low-digit cells; a digit that is full in one tile and empty in the others; keys that differ in
  the top digit only.
* Just over 256 x 4096 points (4096-key tiles) and just over 4 Mi points (6144-key tiles: 683 of them, still the
  two-level look-back; the chained look-back of more than 1024 tiles is C5's 3043 in tests/test_gpu_fullsize.py).
* 17 and 257 tiles again in ticket order (set_build_options(tile_tickets=True)): bitwise the default build.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

xa = pytest.importorskip("xchu_slam_amd")

NT = max(1, min(16, os.cpu_count() or 1))
TILE = 1024
MIN_PTS = 6
FIELDS = ("keys", "npts", "mean", "icov", "centroid")


def _points(cells, seed):
    """One point per row of `cells` (integer i, j, k >= 0), at the cell centre plus an offset of its own below a
    quarter cell (f32: the cell stays the integer part)."""
    rng = np.random.default_rng(seed)
    p = np.ones((len(cells), 4), np.float32)
    p[:, :3] = cells.astype(np.float32) + np.float32(0.5) + rng.uniform(-0.25, 0.25, (len(cells), 3)).astype(np.float32)
    return p


def _anchors(lo, hi):
    """MIN_PTS points in each of two corner cells: they fix the box (and so the key width) and join the KD cloud."""
    return np.repeat(np.array([lo, hi], np.int64), MIN_PTS, axis=0)


def _pool_cells(n, seed, box=(64, 64, 64)):
    """n cells drawn from a pool of about n / 12 cells of the box (most voxels reach MIN_PTS), three key digits wide"""
    rng = np.random.default_rng(seed)
    pool = np.stack([rng.integers(0, b, max(8, n // 12)) for b in box], axis=1)
    cells = pool[rng.integers(0, len(pool), n)]
    cells[:2 * MIN_PTS] = _anchors((0, 0, 0), tuple(b - 1 for b in box))[:min(n, 2 * MIN_PTS)]
    return cells


def _shape_cells(shape):
    n = 5 * TILE + 37
    idx = np.arange(n)
    z = np.zeros(n, np.int64)
    if shape == "one_voxel":
        cells = np.stack([z + 1, z + 2, z + 3], axis=1)
        return np.concatenate([cells, _anchors((0, 0, 0), (63, 63, 63))])
    if shape == "lanes_64_cells":
        cells = np.stack([idx % 64, z, z], axis=1)
        return np.concatenate([cells, _anchors((0, 0, 0), (63, 63, 63))])
    if shape == "digit_per_tile":
        cells = np.stack([idx // TILE, z, z], axis=1)
        return np.concatenate([cells, _anchors((0, 0, 0), (63, 63, 63))])
    if shape == "top_digit_only":
        # a 256 x 256 x 8 box: key = i + 256 j + 65536 k, cells (0, 0, k)
        k = np.random.default_rng(11).integers(0, 8, n)
        cells = np.stack([z, z, k], axis=1)
        return np.concatenate([cells, _anchors((0, 0, 0), (255, 255, 7))])
    raise ValueError(shape)


@functools.lru_cache(maxsize=None)
def _case(name):
    """points of a case and the oracle's KD-cloud leaves, computed once and never changed"""
    import oracle_lib
    oracle_lib.build_oracle()
    kind, _, arg = name.partition(":")
    if kind == "tiles":
        n = int(arg)
        pts = _points(_pool_cells(n, seed=n % 9973), seed=n)
    elif kind == "big":
        n = int(arg)
        rng = np.random.default_rng(n % 9973)
        pool = np.stack([rng.integers(0, 64, n // 64) for _ in range(3)], axis=1)
        cells = pool[rng.integers(0, len(pool), n)]
        cells[:2 * MIN_PTS] = _anchors((0, 0, 0), (63, 63, 63))
        pts = _points(cells, seed=n)
        pts[1::2] = pts[0::2][:len(pts[1::2])]   # duplicates
    else:
        pts = _points(_shape_cells(arg), seed=7)
    pts.setflags(write=False)
    o = oracle_lib.OracleNDT(num_threads=NT, resolution=1.0)
    o.set_target(pts)
    oh, ol = o.grid_header(), o.grid_leaves()
    sel = (ol["npts"] >= MIN_PTS) | (ol["npts"] == -1)
    leaves = {k: ol[k][sel] for k in FIELDS}
    for v in leaves.values():
        v.setflags(write=False)
    return pts, oh, leaves


def _build(pts, **opts):
    g = xa.NormalDistributionsTransform()
    g.setResolution(1.0)
    if opts:
        g.set_build_options(**opts)
    g.setInputTarget(pts)
    return g


def _check(name, **opts):
    pts, oh, ol = _case(name)
    g = _build(pts, **opts)
    gh, gl = g.grid_info(), g.grid_leaves()
    for k in ("min_b", "max_b", "div_b", "divb_mul", "n_leaves", "n_cloud", "overflow"):
        assert oh[k] == gh[k], (name, k, oh[k], gh[k])
    assert len(ol["keys"]) > 0
    for k in FIELDS:
        a, b = ol[k], gl[k]
        if a.shape == b.shape and a.dtype.kind == "f" and a.size:
            print(f"{name} {k}: max |gpu - oracle| = {float(np.max(np.abs(a - b))):.3e}")
        assert np.array_equal(a, b), (name, k)
    return g, gl


TILE_COUNTS = (1, 2, 16, 17, 256, 257, 1024)


@pytest.mark.parametrize("extra", (0, 1))
@pytest.mark.parametrize("tiles", TILE_COUNTS)
def test_tile_counts(tiles, extra):
    _check(f"tiles:{tiles * TILE + extra}")


@pytest.mark.parametrize("shape", ("one_voxel", "lanes_64_cells", "digit_per_tile", "top_digit_only"))
def test_digit_shapes(shape):
    _check(f"shape:{shape}")


def test_4096_key_tiles():
    _check(f"big:{256 * 4096 + 5}")


def test_6144_key_tiles():
    _check(f"big:{(4 << 20) + 3}")


@pytest.mark.parametrize("tiles", (17, 257))
def test_ticket_order_is_the_default_build(tiles):
    name = f"tiles:{tiles * TILE}"
    d, dl = _check(name)
    t, tl = _check(name, tile_tickets=True)
    assert t.build_stats()["tile_tickets"] == 1
    assert d.grid_info() == t.grid_info()
    for k in FIELDS:
        assert np.array_equal(dl[k], tl[k]), k
