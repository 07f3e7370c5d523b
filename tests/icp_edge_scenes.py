"""Scenes of tests/test_gpu_icp_edges.py and the reference-side facts they rest on (no GPU): tie lattices, degenerate
target shapes, queries on every side of the grid, the index geometry of the nearest-neighbour build, sparse partner
clouds for the estimate's degenerate branches.  Every builder is deterministic; tests/test_icp_restate.py asserts the
input conditions the device tests depend on, so a scene that stops meeting one fails without a GPU."""
import numpy as np

import icp_restate as R

F32 = np.float32
MAP_OFFSET = np.array([512.0, -384.0, 16.0])  # a map-frame position: every integer offset from it is exact in f32
K_BLOCK = 8                                   # cells per block side of the index (kFitBlockCells = 8^3)
MAX_KEYS = 1 << 25                            # kFitMaxKeys: the block-major key range the index doubles its cell to fit


# ---------------------------------------------------------------------------------------------- index geometry
def index_geometry(target, resolution):
    """The nearest-neighbour index's cell and grid for a target, by the arithmetic of its build (voxel_build.hip, layout
    1, all in f32): cell = resolution, doubled until nbk0 * nbk1 * nbk2 * 512 <= 2^25 with nbk = ceil(div / 8) and
    div = floor(max / cell) - floor(min / cell) + 1.  Returns dict(cell, doublings, min_b, div_b, nbk, keys) with
    `keys` the key range of every cell size tried."""
    P = np.asarray(target, F32)[:, :3]
    mn, mx = P.min(0), P.max(0)
    cell = F32(resolution)
    keys = []
    for doublings in range(64):
        inv = F32(1.0) / cell
        min_b = np.floor(mn * inv).astype(np.int64)
        max_b = np.floor(mx * inv).astype(np.int64)
        div_b = max_b - min_b + 1
        nbk = (div_b + 7) >> 3
        keys.append(int(nbk[0] * nbk[1] * nbk[2] * K_BLOCK ** 3))
        if keys[-1] <= MAX_KEYS:
            return {"cell": cell, "inv": inv, "doublings": doublings, "min_b": min_b, "div_b": div_b, "nbk": nbk, "keys": keys}
        cell = cell * F32(2.0)
    raise AssertionError("no cell size fits")


def cells_of(points, geo):
    """Grid cell of every point (relative to the grid's minimum, as the walk computes it) and its block-major key."""
    P = np.asarray(points, F32)[:, :3]
    c = (np.floor(P * geo["inv"]) - geo["min_b"].astype(F32)).astype(np.int64)
    b = c >> 3
    nbk = geo["nbk"]
    key = ((b[:, 2] * nbk[1] + b[:, 1]) * nbk[0] + b[:, 0]) * K_BLOCK ** 3 + (((c[:, 2] & 7) << 6) | ((c[:, 1] & 7) << 3) | (c[:, 0] & 7))
    return c, key


def at_minimum(X, P):
    """(n, m) mask of the target points at each query's minimal f32 distance (small clouds only)."""
    d2 = R.l2_simple_f32(np.asarray(P, F32)[None, :, :3], np.asarray(X, F32)[:, None, :3])
    return d2 == d2.min(1)[:, None]


def tie_census(X, P, resolution):
    """Reference-side facts of a tie scene: `tied` = queries with two or more target points at the minimum; `not_first`
    = those of them whose winner (the lowest index) is not the candidate a walk in cell-key order meets first (the
    lowest (cell key, index))."""
    geo = index_geometry(P, resolution)
    _, key = cells_of(P, geo)
    at = at_minimum(X, P)
    m = len(P)
    winner = at.argmax(1)
    rank = key * m + np.arange(m)  # (key, index) as one number
    first = np.where(at, rank[None, :], np.iinfo(np.int64).max).argmin(1)
    tied = at.sum(1) > 1
    return {"tied": tied, "not_first": tied & (winner != first), "winner": winner, "first": first, "geo": geo}


# ---------------------------------------------------------------------------------------------- tie scenes
def lattice_scene(seed=0, nx=12, ny=12, nz=6, n_dup=200, spacing=1):
    """Target: the nx x ny x nz integer lattice at MAP_OFFSET plus n_dup repeated lattice points, shuffled (every value
    exact in f32; at resolution 1.0 every point lies on a cell face).  Queries: the cell centres (8 candidates in 8
    cells), the midpoints of the x edges (2 candidates), and 288 lattice points, the repeated ones among them (d2 = 0,
    the tie inside one cell).  Returns (target, queries, kinds) with kinds 0 / 1 / 2 per query.
    spacing=1: the 8 candidates of a centre sit in 8 cells that 8 different lanes of the team scan, so only NnArg::team
    orders them.  spacing=2: the centres are cell corners (face distance 0) with candidates at d2 = 3 in the cells at
    offsets (+-1, +-1, +-1); the radius-1 cube cannot conclude, and in both cubes two of the eight fall to one lane
    (cells 2 and 18, 8 and 24 of the 27; 33 and 81, 43 and 91 of the 125), so NnArg::take's own tie branch orders them and
    the second cube meets every candidate again."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    dup = rng.choice(len(g), n_dup, replace=False)
    tgt = np.concatenate([g, g[dup]])
    tgt = tgt[rng.permutation(len(tgt))] + MAP_OFFSET
    centres = g[(g[:, 0] < nx - 1) & (g[:, 1] < ny - 1) & (g[:, 2] < nz - 1)] + 0.5
    edges = g[g[:, 0] < nx - 1] + np.array([0.5, 0.0, 0.0])
    rest = np.setdiff1d(np.arange(len(g)), dup)
    on = g[np.concatenate([dup, rng.choice(rest, 288 - n_dup, replace=False)])]
    tgt = (tgt - MAP_OFFSET) * spacing + MAP_OFFSET
    q = np.concatenate([centres, edges, on]) * spacing + MAP_OFFSET
    kinds = np.concatenate([np.zeros(len(centres), int), np.ones(len(edges), int), np.full(len(on), 2)])
    tgt32, q32 = tgt.astype(F32), q.astype(F32)
    assert np.array_equal(tgt32.astype(np.float64), tgt) and np.array_equal(q32.astype(np.float64), q)  # exact in f32
    return tgt32, q32, kinds


def sparse_tie_scene(seed=1):
    """A sparse lattice whose ties fall to the block-shell phase: x in {2, 11, 20, 29, 38} (spacing 9), y and z in
    {2, 7, ..., 37} (spacing 5), 320 points, shuffled.  Queries: the x midpoints (6.5, 15.5, ...: neighbours 4.5 away
    on both sides, beyond the radius-2 cube at cells of 1.0 and 0.5, and in different 8^3 blocks) and the y midpoints
    (2.5 away: one neighbour inside the radius-2 cube at resolution 1.0, one outside).  Returns (target, queries,
    is_x_midpoint)."""
    rng = np.random.default_rng(seed)
    xs, ys = 2.0 + 9.0 * np.arange(5), 2.0 + 5.0 * np.arange(8)
    g = np.stack(np.meshgrid(xs, ys, ys, indexing="ij"), -1).reshape(-1, 3)
    tgt = g[rng.permutation(len(g))]
    qx = g[g[:, 0] < xs[-1]] + np.array([4.5, 0.0, 0.0])
    qy = g[g[:, 1] < ys[-1]] + np.array([0.0, 2.5, 0.0])
    q = np.concatenate([qx, qy])
    return tgt.astype(F32), q.astype(F32), np.arange(len(q)) < len(qx)


# ---------------------------------------------------------------------------------------------- target shapes
def shape_targets(seed=2):
    """The four degenerate targets, all away from the origin on the negative side of y."""
    rng = np.random.default_rng(seed)
    one = np.array([[3.25, -7.5, 1.75]], F32)
    in_cell = (np.array([10.0, -21.0, 4.0]) + rng.uniform(0.05, 0.95, (40, 3))).astype(F32)
    in_cell[7] = in_cell[3]  # a repeated point
    sheet = np.column_stack([rng.uniform(-12.0, 18.0, 600), rng.uniform(-33.0, -3.0, 600), np.full(600, 0.5)]).astype(F32)
    return {"one_point": one, "copies": np.repeat(one, 500, 0), "one_cell": in_cell, "one_layer": sheet}


def queries_around(target, resolution, seed=3, n_inside=40, per_side=6):
    """Queries inside the target's grid and outside it on all six sides at 1, 2, 3 and 20 cells from the grid's outer
    cell (r0 <= 2: the cubes run first; r0 > 2: block shells at once), the other two coordinates inside the grid or up
    to 2 cells off it."""
    rng = np.random.default_rng(seed)
    geo = index_geometry(target, resolution)
    cell = float(geo["cell"])
    lo = geo["min_b"].astype(np.float64) * cell
    hi = lo + geo["div_b"] * cell
    q = [rng.uniform(lo, hi, (n_inside, 3))]
    for axis in range(3):
        for side in (-1, 1):
            for off in (1, 2, 3, 20):
                p = rng.uniform(lo - 2 * cell, hi + 2 * cell, (per_side, 3))
                frac = rng.uniform(0.05, 0.95, per_side) * cell
                p[:, axis] = lo[axis] - off * cell + frac if side < 0 else hi[axis] + (off - 1) * cell + frac
                q.append(p)
    q = np.concatenate(q).astype(F32)
    c, _ = cells_of(q, geo)
    out = np.maximum(np.maximum(-c, c - geo["div_b"] + 1), 0).max(1)  # the walk's r0
    return q, c, out, geo


# ---------------------------------------------------------------------------------------------- doubled cell
def doubled_cell_scene(seed=4, n=2000):
    """Two n-point clusters (10 m squares, z within 0.05..0.75: one block at either cell size) whose centres are 400 m
    apart, (290, 275) m: at resolution 0.1 the grid is 2951 x 2801 x 8 cells = 369 x 351 x 1 blocks = 6.6e7 keys, over
    2^25 = 3.4e7, so the index doubles its cell to 0.2 (185 x 176 x 1 blocks, 1.7e7 keys).  Queries: cluster points
    moved by 0.3 m of noise, and 8 points on the line between the clusters (hundreds of empty block shells)."""
    rng = np.random.default_rng(seed)
    a = np.column_stack([rng.uniform(0.0, 10.0, (n, 2)), rng.uniform(0.05, 0.75, n)])
    b = np.column_stack([rng.uniform(0.0, 10.0, (n, 2)) + [290.0, 275.0], rng.uniform(0.05, 0.75, n)])
    tgt = np.concatenate([a, b])
    tgt = tgt[rng.permutation(len(tgt))].astype(F32)
    near = tgt[rng.choice(len(tgt), 1500, replace=False)].astype(np.float64) + rng.normal(0.0, 0.3, (1500, 3))
    t = rng.uniform(0.1, 0.9, 8)[:, None]
    between = np.array([5.0, 5.0, 0.4]) + t * np.array([290.0, 275.0, 0.0]) + rng.normal(0.0, 1.0, (8, 3))
    return tgt, np.concatenate([near, between]).astype(F32)


# ---------------------------------------------------------------------------------------------- estimates
def rigid(tx, ty, tz, deg, axis=(0.0, 0.0, 1.0)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = [tx, ty, tz]
    return T


def sigma_of(P, Q):
    """The estimate's cross-covariance (Q the matched target points, P the source), f64."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    return (Q - Q.mean(0)).T @ (P - P.mean(0)) / len(P)


def planar_partner_scene(seed, z_noise, n=120, spacing=4.0):
    """Partner clouds on a jittered planar grid (spacing 4 m, jitter 0.5 m: neighbours stay 3 to 5 m apart): the source
    is the target's x, y moved back by a 0.3 m / 2 deg in-plane displacement; z of source and of target are independent
    noise of `z_noise` (0: both exactly 0, a rank-2 cross-covariance)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n]
    xy = (ij - side / 2) * spacing + rng.uniform(-0.5, 0.5, (n, 2))
    tgt = np.column_stack([xy, rng.normal(0.0, z_noise, n) if z_noise else np.zeros(n)])
    inv = np.linalg.inv(rigid(0.2, -0.2, 0.0, 2.0))
    sxy = xy @ inv[:2, :2].T + inv[:2, 3]
    src = np.column_stack([sxy, rng.normal(0.0, z_noise, n) if z_noise else np.zeros(n)])
    return tgt.astype(F32), src.astype(F32)


def reflection_scene(z_noise=1e-3, seeds=range(64)):
    """The first planar_partner_scene whose first-iteration cross-covariance has a negative determinant (independent z
    noise makes its third singular direction a coin toss): Umeyama's sign must flip there.  Returns (target, source,
    seed)."""
    for seed in seeds:
        tgt, src = planar_partner_scene(seed, z_noise)
        idx, _, _ = R.nearest_bruteforce(src, tgt)
        if np.array_equal(idx, np.arange(len(src))) and np.linalg.det(sigma_of(src, tgt[idx])) < 0:
            return tgt, src, seed
    raise AssertionError("no seed with det(sigma) < 0")


def collinear_scene(seed=6, n=40, spacing=5.0):
    """Rank 1: partners on one line (direction (2, 1, 0.5), 5 m apart), the source moved 0.3 m along and across it."""
    rng = np.random.default_rng(seed)
    d = np.array([2.0, 1.0, 0.5]) / np.linalg.norm([2.0, 1.0, 0.5])
    s = (np.arange(n) - n / 2) * spacing + rng.uniform(-0.5, 0.5, n)
    tgt = np.array([7.0, -3.0, 1.0]) + s[:, None] * d
    src = tgt + 0.2 * d + np.array([-0.1, 0.2, 0.0])
    return tgt.astype(F32), src.astype(F32)


def one_target_scene(seed=7, n=50):
    """Rank 0: every source point matches the one target point."""
    rng = np.random.default_rng(seed)
    return np.array([[4.0, -2.5, 1.0]], F32), (np.array([4.0, -2.5, 1.0]) + rng.uniform(-3.0, 3.0, (n, 3))).astype(F32)


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


def residual_rms(T, P, Q):
    """Root mean squared residual |T p - q| over the pairs, f64."""
    T, P, Q = np.asarray(T, np.float64), np.asarray(P, np.float64), np.asarray(Q, np.float64)
    r = P @ T[:3, :3].T + T[:3, 3] - Q
    return float(np.sqrt((r * r).sum(1).mean()))


def residual_delta(P, T):
    """How far one f32 ulp in each entry of T moves a coordinate: 4 * 2^-23 * max|p| + ulp32(max|t|), t the translation
    of T (the restatement's)."""
    return 4.0 * 2.0 ** -23 * float(np.max(np.abs(P))) + ulp32(float(np.max(np.abs(np.asarray(T)[:3, 3]))))
