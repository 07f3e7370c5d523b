"""Inputs for the front-end edge tests (test_front_end_cases.py on the CPU, test_gpu_front_end_edges.py on the
device): structured clouds that reach the branches of k_crop_flags, k_sor_knn, k_ror_keep and the neighbour index
which a random LiDAR-like scan never does.  Every case is a named generator returning (cloud (N, 4) float32, kwargs
for filter_scan); `CASES` lists every (case, parameter set) once, and `reference` computes the brute-force oracle
result once per entry and keeps it.

Device path per family (xchu_slam_amd/csrc/front_end.hip):
  lattice        points on index-cell faces, tied distances: the merge's tie rule and pop, count_le at exactly
                 ring * cell, k_ror_keep's strict < at exactly the radius; lane lists of 32 (mean_k <= 31) and 64
  clusters       neighbours 15+ block shells away (stop bound (8 r) cell - slack), lists of 32 and 64
  shell_bound    a query whose nearest points lie one block shell further out than other, farther points: only the
                 stop bound (8 r) cell - slack keeps the shell search going
  line           an index one cell thick in two axes (exit at ring >= rmax, bmax of 0 in y and z)
  tiny           n_voxel == mean_k (pass-through), == mean_k + 1 (the search runs to bmax), mean_k 1 and 63
  offset         coordinates near 3600 m: a coarse f32 grid, the slack term of the stop bound is not negligible
  scattered      leaf sweep; leaf 0.03 and 0.02 and ROR radius 0.05: the index doubles its cell (header cell used)
  overflow_dups  VoxelGrid overflow: output = crop copy, exact duplicates (several zero distances) reach the k-NN
  crop_edges     r == r_min, r == r_max and their float neighbours, +-inf, -0.0, NaN coordinates, NaN intensity
"""
from collections import namedtuple

import numpy as np

# keeps: what the outlier stage leaves of the voxel points, "some" (at least one kept, at least one dropped) unless the
#   geometry of the case fixes it to "all" or "none" (reasons beside the entries of CASES)
# grid_ok: the oracle's own hash-grid search (brute=False) finishes on it in reasonable time
Case = namedtuple("Case", "id gen kw keeps grid_ok")


def _with_intensity(xyz, seed):
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, np.float32)
    return np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1)).astype(np.float32)], 1)


def lattice():
    """0.75 m lattice over [-12, 12)^2 x [0, 3) minus hypot(x, y) <= 1.2: 4060 points, one per 0.5 m voxel.  0.75 is
    half the index cell at leaf 0.5 (1.5 m), so every other point lies on a cell face and most distances tie."""
    a = np.arange(-12.0, 12.0, 0.75)
    z = np.arange(0.0, 3.0, 0.75)
    g = np.stack(np.meshgrid(a, a, z, indexing="ij"), -1).reshape(-1, 3)
    g = g[np.hypot(g[:, 0], g[:, 1]) > 1.2]
    assert len(g) == 4060
    return _with_intensity(g, 101)


def clusters():
    """A 3000-point blob, a 9-point cluster ~180 m from it and two lone points: the cluster and the lone points find
    their mean_k + 1 neighbours only in the blob, more than ten 8x8x8-cell block shells away."""
    rng = np.random.default_rng(102)
    blob = rng.uniform([-8, -8, 0], [8, 8, 2], (3000, 3))
    g = np.stack(np.meshgrid(np.arange(3) * 0.7, np.arange(3) * 0.7, indexing="ij"), -1).reshape(-1, 2)
    small = np.concatenate([g + [151.0, 101.0], np.full((9, 1), 20.5)], 1) + rng.uniform(-0.05, 0.05, (9, 3))
    lone = np.array([[-200.0, 30.0, -5.0], [10.0, -250.0, 40.0]])
    return _with_intensity(np.concatenate([blob, small, lone]), 103)


def shell_bound():
    """The block-shell stop bound at its edge, in one dimension (index cell 1.5 m at leaf 0.5, blocks of 8 cells = 12 m,
    cell 0 starting at x = 3.0 through the anchor point at x = 3.25).  The query Q sits in the first cell of block 3;
    group A (8 voxel centres) in the last cell of block 5, 23 cells away in shell 2; group B (8 voxel centres) in the
    last cell of block 0, 16.7 cells away but in shell 3.  After shell 2 the search holds A's 8 points, all beyond the
    bound of 16 cells, so it must go on to shell 3 and answer with B; a bound one shell too generous stops at A."""
    g = np.stack(np.meshgrid([0.0, 0.5], [3.25, 3.75], [0.25, 0.75], indexing="ij"), -1).reshape(-1, 3)
    a, b = g + [73.75, 0, 0], g + [14.25, 0, 0]
    return _with_intensity(np.concatenate([[[3.25, 3.25, 0.25]], b, [[39.25, 3.25, 0.25]], a]), 112)


def line():
    """80 points on a line along x: the neighbour index is one cell thick in y and z."""
    x = 2.0 + 0.6 * np.arange(80)
    return _with_intensity(np.stack([x, np.full(80, 3.0), np.zeros(80)], 1), 104)


def tiny(nv):
    """nv points snapped to distinct 0.5 m voxel centres of a small box clear of the crop radii."""
    rng = np.random.default_rng(105)
    cells = np.stack(np.meshgrid(np.arange(8, 14), np.arange(-3, 3), np.arange(0, 3), indexing="ij"), -1).reshape(-1, 3)
    pick = cells[rng.permutation(len(cells))[:nv]]
    return _with_intensity((pick + 0.5) * 0.5, 106)


def tiny_pair():
    """Two voxel centres (0.5, 0.5, 1.0) apart for mean_k = 1: both distances are d = (float)sqrt(1.5).  The variance
    is then the rounding residue 2 (fl32(d d) - d d) = 2.0e-8 > 0, which two addends define in any summation order, so
    the threshold sits 1.2e-4 (relative) above both distances and both points are kept.  (Many other offsets, such as
    (0.5, 1.0, 0), give a negative residue and a NaN threshold.)"""
    return _with_intensity(np.array([[5.25, 3.25, 0.25], [5.75, 3.75, 1.25]]), 107)


def offset():
    """4000 points in a 20 x 20 x 3 box ~3600 m from the sensor (f32 spacing 2.4e-4 m)."""
    rng = np.random.default_rng(108)
    p = rng.uniform([0, 0, 0], [20, 20, 3], (4000, 3)) + [3000.0, -2000.0, 500.0]
    return _with_intensity(p, 109)


def scattered():
    """6000 points in [-30, 30]^2 x [-2, 6], 90 % of them on the plane z = 0."""
    rng = np.random.default_rng(110)
    p = rng.uniform([-30, -30, -2], [30, 30, 6], (6000, 3))
    p[rng.random(6000) < 0.9, 2] = 0.0
    return _with_intensity(p, 111)


def overflow_dups():
    """The first 1500 scattered points plus the first 300 of them again: at leaf 1e-4 VoxelGrid overflows, the output
    is the crop copy, and the duplicates reach the k-NN with zero distances."""
    s = scattered()
    return np.concatenate([s[:1500], s[:300]])


# the rows of crop_edges that the front end keeps (CROP_EDGES_KEPT indexes the table below)
CROP_EDGES_KEPT = [3, 6, 2, 12, 13]


def crop_edges():
    """14 rows at the edges of the crop: r == r_min and r == r_max (strict comparisons, dropped), their float
    neighbours inside (kept), (0.6, 0.8) whose f32 squares sum above 1 in double (kept), non-finite coordinates
    (dropped), -0.0 (kept) and a NaN intensity (kept: removeNaNFromPointCloud looks at x, y, z only)."""
    one, sixty = np.float32(1.0), np.float32(60.0)
    inf, nan = np.inf, np.nan
    rows = [
        [1, 0, 0, 0.1], [0, -1, 0, 0.2], [0.6, 0.8, 0, 0.3], [np.nextafter(one, np.float32(2)), 0, 0, 0.4],
        [60, 0, 0, 0.5], [36, 48, 1, 0.6], [np.nextafter(sixty, np.float32(0)), 0, 0, 0.7],
        [inf, 5, 0, 0.8], [5, -inf, 0, 0.9], [5, 5, inf, 1.0], [nan, 5, 0, 1.1], [5, 5, nan, 1.2],
        [-0.0, 2, 0, 1.3], [3, 4, 0, nan],
    ]
    return np.array(rows, np.float32)


def _cases():
    out = []

    def add(cid, gen, keeps="some", grid_ok=False, **kw):
        out.append(Case(cid, gen, kw, keeps, grid_ok))

    for k in (6, 30, 31, 32, 63):
        add(f"lattice-sor{k}", lattice, grid_ok=True, mean_k=k)
    # (0.75, 7) and (0.1, 2): 0.75^2 = 0.5625 is exact and the test is <, so only the point itself counts and nothing is
    # kept; min 1 keeps everything (the point itself is a neighbour); (3.0, 40) keeps everything too: even a corner
    # point has 15 + 15 + 13 + 8 = 51 lattice points with i^2 + j^2 + k^2 < 16 in its octant
    for rad, mn, keeps in ((0.8, 5, "some"), (0.75, 7, "none"), (0.75, 1, "all"), (3.0, 40, "all"), (0.1, 1, "all"),
                           (0.1, 2, "none")):
        add(f"lattice-ror{rad}-{mn}", lattice, keeps=keeps, grid_ok=True, outlier_method=1, ror_radius=rad, ror_min_neighbors=mn)
    for k in (30, 63):
        add(f"clusters-sor{k}", clusters, r_max=400.0, mean_k=k)
    add("shell_bound-sor6", shell_bound, grid_ok=True, r_max=400.0, mean_k=6)
    for k in (30, 63):
        add(f"line-sor{k}", line, grid_ok=True, mean_k=k)
    for nv, k in ((30, 30), (31, 30), (32, 30), (64, 63), (65, 63)):
        add(f"tiny-nv{nv}-sor{k}", lambda nv=nv: tiny(nv), keeps="all" if nv == k else "some", grid_ok=True, mean_k=k)
    # two points have one and the same distance: both kept or both dropped, so this case cannot remove one
    add("tiny-nv2-sor1", tiny_pair, keeps="all", grid_ok=True, mean_k=1)
    add("offset-sor30", offset, r_min=3000.0, r_max=5000.0)
    for leaf in (0.1, 0.3, 2.0):
        add(f"scattered-leaf{leaf}", scattered, grid_ok=True, leaf=leaf)
    # leaf 0.03: index base cell 0.09 m; 60 m / 0.09 = 667 cells = 84 blocks of 8 in x and y, 8 m / 0.09 = 89 cells =
    # 12 blocks in z; 84 * 84 * 12 * 512 = 43.4e6 keys > 2^25 = 33.6e6, so the cell doubles to 0.18 m.  VoxelGrid itself
    # (2000 * 2000 * 267 = 1.07e9 voxels < 2^31) does not overflow.
    add("scattered-leaf0.03", scattered, leaf=0.03)
    # leaf 0.02: index base cell 0.06 m; 60 m / 0.06 = 1000 cells = 125 blocks in x and y, 8 m / 0.06 = 134 cells = 17
    # blocks in z; 125 * 125 * 17 * 512 = 136e6 keys > 2^25, so the cell doubles to 0.12 m (63 * 63 * 9 * 512 = 18.3e6
    # fits).  At this leaf VoxelGrid overflows as well (3000 * 3000 * 400 = 3.6e9 voxels > 2^31), so the k-NN runs on
    # the crop copy.
    add("scattered-leaf0.02", scattered, leaf=0.02)
    # ROR index base cell 1.01 * radius: at 0.05 that is 0.0505 m, 60 m -> 1189 cells = 149 blocks, 8 m -> 159 cells =
    # 20 blocks; 149 * 149 * 20 * 512 = 227e6 keys > 2^25: doubled to 0.101 m (75 * 75 * 10 * 512 = 28.8e6)
    # (0.05, 2) keeps nothing at leaf 0.5 (no two voxel means lie within 5 cm); at leaf 0.03, where the points stay
    # apart, it keeps the few close pairs
    for rad, mn, keeps in ((0.8, 5, "some"), (0.2, 2, "some"), (3.0, 40, "some"), (0.05, 1, "all"), (0.05, 2, "none")):
        add(f"scattered-ror{rad}-{mn}", scattered, keeps=keeps, outlier_method=1, ror_radius=rad, ror_min_neighbors=mn)
    add("scattered-leaf0.03-ror0.05-2", scattered, leaf=0.03, outlier_method=1, ror_radius=0.05, ror_min_neighbors=2)
    add("overflow_dups-sor30", overflow_dups, leaf=1e-4, r_max=100.0)
    add("overflow_dups-ror", overflow_dups, leaf=1e-4, r_max=100.0, outlier_method=1)
    # five rows survive the crop: fewer than mean_k, the outlier stage passes them through
    add("crop_edges", crop_edges, keeps="all")
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]

_clouds = {}
_refs = {}


def cloud_of(case):
    """The case's input cloud, generated once and read-only."""
    if case.id not in _clouds:
        a = np.ascontiguousarray(case.gen(), np.float32)
        a.setflags(write=False)
        _clouds[case.id] = a
    return _clouds[case.id]


def reference(oracle, case):
    """(out, distances, thr[3], n_voxel) of the oracle's brute-force front end, computed once per case."""
    if case.id not in _refs:
        out, dist, thr, nv = oracle.filter_scan(cloud_of(case), brute=True, is_dense=False, **case.kw)
        for a in (out, dist, thr):
            a.setflags(write=False)
        _refs[case.id] = (out, dist, thr, nv)
    return _refs[case.id]


def bits(a):
    """Rows as uint32 words: compares NaN payloads and the sign of zero."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
