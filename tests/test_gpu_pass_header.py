"""The direct passes across leaf sizes, lookup structures, cell faces and header changes.

The leading-tail kernel (k_pass_lead) reads the grid header behind its control step and hands the state on with
partials_pending set in the word workgroup 0 writes out; the last-workgroup-tail kernel (k_pass_direct) reads the header
behind its state check.  Both take the cell index from floor(x / leaf).  What is pinned here: leaf sizes that are powers
of two (1.0, 0.5, 2.0) and not (0.7, 1.3); the dense cell grid and the hash grid; a target with no usable voxel (the
header's `empty` flag); source points exactly on cell faces, one ulp to either side, one cell outside the box and far
outside it; DIRECT1 / DIRECT7 / DIRECT26, the multi-tile leading-tail kernel on a 200 000-point source; and a context
whose second target has another leaf size, box and lookup structure than its first.

Bars against the oracle are test_gpu_parity.py's: the pair count of every pass exact, every per-pass parameter vector
within X_TOL = 1e-12, the same iteration count.  The leading-tail chain against the last-workgroup tails
(ndt_set_pass_options(lead_tail = 0)) is bit for bit where both run one geometry (test_gpu_lead.py).

ndt_grid_info does not report the lookup structure itself; it reports div_b, and a build is dense exactly when
div_b[0] * div_b[1] * div_b[2] fits the cell grid's allocation, 16 Mi cells for a context that has seen no larger grid
(host_target.hip grow_grid, voxel_build.hip header_body) — every context here is fresh when that matters."""
import numpy as np
import pytest

from helpers import TF_TOL, X_TOL, small_pair

pytestmark = pytest.mark.gpu

xa = pytest.importorskip("xchu_slam_amd")
from xchu_slam_amd import synth  # noqa: E402

GRID_ALLOC_CELLS = 16 << 20
POW2_LEAVES = [1.0, 0.5, 2.0]      # x / leaf is exact up to the exponent
OTHER_LEAVES = [0.7, 1.3]


def scene(seed=3, n_source=2000, leaf=1.0):
    """~25 k target points and a LiDAR-like source (helpers.small_pair on a smaller map), the whole scene scaled by the
    leaf size: every leaf size sees the voxel occupancy of the 1 m case (up to f32 rounding of the scaled points)."""
    p = small_pair(seed=seed, half=30.0, n_source=n_source, max_range=22.0)
    guess, true = p.guess.copy(), p.true_pose.copy()
    guess[:3, 3] *= leaf
    true[:3, 3] *= leaf
    return synth.Pair(target=(p.target * np.float32(leaf)).astype(np.float32), source=(p.source * np.float32(leaf)).astype(np.float32),
                      true_pose=true, guess=guess)


def two_clusters(pair, leaf):
    """pair's target plus a small second cluster 300 leaf sizes away on every axis: > 2.7e7 cells, a hash grid."""
    rng = np.random.default_rng(17)
    far = (rng.uniform(0.0, 2.0 * leaf, (400, 3)) + 300.0 * leaf + np.asarray(pair.target, np.float32).max(0)).astype(np.float32)
    return np.concatenate([pair.target, far]).astype(np.float32)


def device(target, source, lead_tail=True, **prm):
    g = xa.NormalDistributionsTransform()
    g.set_pass_options(lead_tail=lead_tail)
    for k, v in prm.items():
        setattr(g._params, k, v)
    g._push()
    g.setInputTarget(target)
    g.setInputSource(source)
    return g


def record(g, guess):
    g.align(guess, want_output=False)
    r = g.result()
    return {"tf": r["final_tf"].astype(np.float64).ravel().tolist(), "iters": r["nr_iterations"], "converged": r["converged"],
            "passes": r["n_passes"], "hist": g.history()}


def flat(hist):
    return [[h["kind"], h["score"], h["pairs"]] + h["x"].tolist() + h["g"].tolist() + h["H"].ravel().tolist() for h in hist]


def assert_bitwise(a, b, what):
    assert a["iters"] == b["iters"] and a["passes"] == b["passes"] and a["converged"] == b["converged"], what
    assert a["tf"] == b["tf"], what
    fa, fb = flat(a["hist"]), flat(b["hist"])
    assert len(fa) == len(fb) > 0, what
    for k, (ra, rb) in enumerate(zip(fa, fb)):
        assert ra == rb, (what, k)


def assert_oracle(oracle, target, source, guess, rec, what, **prm):
    o = oracle.OracleNDT(num_threads=1, **prm)
    o.set_target(target)
    o.set_source(source)
    ro = o.align(guess)
    ho = o.history()
    assert rec["iters"] == ro["nr_iterations"] and rec["converged"] == ro["converged"], what
    assert len(ho) == len(rec["hist"]), what
    for k, (a, b) in enumerate(zip(ho, rec["hist"])):
        assert a["kind"] == b["kind"], (what, k)
        assert a["pairs"] == b["pairs"], (what, k, a["pairs"], b["pairs"])
        assert np.max(np.abs(a["x"] - b["x"])) <= X_TOL, (what, k)
    assert np.max(np.abs(np.asarray(rec["tf"]).reshape(4, 4) - ro["final_tf"])) < TF_TOL, what
    o.close()
    return ho


def both_chains(oracle, target, source, guess, what, expect_pairs=True, **prm):
    lead = device(target, source, True, **prm)
    last = device(target, source, False, **prm)
    a, b = record(lead, guess), record(last, guess)
    lead.close()
    last.close()
    assert_bitwise(a, b, what)
    ho = assert_oracle(oracle, target, source, guess, a, what, **prm)
    if expect_pairs:
        assert ho[0]["pairs"] > 0, what
    return a


@pytest.mark.parametrize("leaf", POW2_LEAVES + OTHER_LEAVES)
def test_leaf_sizes_dense_grid(oracle, leaf):
    pair = scene(leaf=leaf)
    prm = dict(resolution=leaf, step_size=0.1, trans_eps=0.0, max_iter=5, search=xa.DIRECT7)
    g = device(pair.target, pair.source, **prm)
    d = g.grid_info()["div_b"]
    g.close()
    assert d[0] * d[1] * d[2] <= GRID_ALLOC_CELLS  # the dense cell grid
    both_chains(oracle, pair.target, pair.source, pair.guess, f"leaf {leaf}", **prm)


@pytest.mark.parametrize("leaf", [1.0, 0.5, 0.7])
def test_leaf_sizes_hash_grid(oracle, leaf):
    pair = scene(seed=5, leaf=leaf)
    tgt = two_clusters(pair, leaf)
    prm = dict(resolution=leaf, step_size=0.1, trans_eps=0.0, max_iter=5, search=xa.DIRECT7)
    g = device(tgt, pair.source, **prm)   # a fresh context: the cell grid holds 16 Mi cells
    d = g.grid_info()["div_b"]
    g.close()
    assert d[0] * d[1] * d[2] > GRID_ALLOC_CELLS  # not dense: the open-addressing hash
    both_chains(oracle, tgt, pair.source, pair.guess, f"hash, leaf {leaf}", **prm)


@pytest.mark.parametrize("search", [xa.DIRECT7, xa.DIRECT1])
def test_empty_grid(oracle, search):
    """No voxel reaches min_points_per_voxel: the header's `empty` flag — no pairs in any pass, and the align ends as
    the oracle's does (zero derivatives)."""
    rng = np.random.default_rng(2)
    ijk = np.stack(np.meshgrid(np.arange(-10, 10), np.arange(-10, 10), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 3)
    reps = np.repeat(ijk, 2, axis=0).astype(np.float32)     # two points per cell, min_points_per_voxel is 6
    tgt = (reps + rng.uniform(0.1, 0.9, reps.shape)).astype(np.float32)
    src = rng.uniform([-8, -8, -1.5], [8, 8, 2.5], (1500, 3)).astype(np.float32)
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=0.01, max_iter=5, search=search)
    g = device(tgt, src, **prm)
    info = g.grid_info()
    g.close()
    assert info["n_leaves"] == len(ijk) and info["n_cloud"] == 0
    rec = both_chains(oracle, tgt, src, np.eye(4), "empty grid", expect_pairs=False, **prm)
    assert all(h["pairs"] == 0 for h in rec["hist"])


def face_points(leaf):
    """Source points on cell faces under the identity guess: k * leaf and its two f32 neighbours on one axis (the other
    two coordinates inside a cell), all three coordinates on faces, points one cell outside the target's box and far
    outside it."""
    f = np.float32
    vals = []
    for k in (-4, -3, -1, 0, 1, 2, 4):
        c = f(k) * f(leaf)
        vals += [c, np.nextafter(c, f(np.inf)), np.nextafter(c, f(-np.inf))]
    vals = np.array(vals, np.float32)
    mid = np.array([0.37, -1.61, 0.83], np.float32) * f(leaf)
    pts = []
    for a in range(3):
        for v in vals:
            p = mid.copy()
            p[a] = v
            pts.append(p)
    for v in vals:
        pts.append(np.array([v, v, np.clip(v, f(-2 * leaf), f(2 * leaf))], np.float32))
    box = np.array([4.0, 4.0, 2.0], np.float32) * f(leaf)
    for s in (-1.0, 1.0):
        for a in range(3):
            p = mid.copy()
            p[a] = f(s) * (box[a] + f(0.5 * leaf))          # one cell outside the box: its -+ neighbour is a grid cell
            pts.append(p)
            q = mid.copy()
            q[a] = f(s) * (box[a] + f(1.5 * leaf))          # two cells outside: no neighbour
            pts.append(q)
            r = mid.copy()
            r[a] = f(s) * f(1000.0 * leaf)
            pts.append(r)
    pts.append(np.array([3.0e7, -3.0e7, 1.0e9], np.float32) * f(leaf))   # cell indices still within int32
    return np.array(pts, np.float32)


@pytest.mark.parametrize("leaf", POW2_LEAVES)
def test_face_and_border_points(oracle, leaf):
    """Per point, the neighbour set of one pass at the identity equals the
    oracle's — its size exactly, and the score of that point alone (a sum over exactly those voxels) within 1e-9, the
    single-pass bar; the whole cloud's first pass through both chains has the oracle's pair count."""
    rng = np.random.default_rng(9)
    tgt = (rng.uniform([-4, -4, -2], [4, 4, 2], (20000, 3)) * leaf).astype(np.float32)   # every cell of the box filled
    pts = face_points(leaf)
    prm = dict(resolution=leaf, step_size=0.1, trans_eps=0.0, max_iter=1)
    eye, p0 = np.eye(4, dtype=np.float32), np.zeros(6)
    for search in (xa.DIRECT7, xa.DIRECT1):
        o = oracle.OracleNDT(num_threads=1, search=search, **prm)
        o.set_target(tgt)
        keys, cnt = o.neighbors(pts, search)
        assert cnt.max() >= (7 if search == xa.DIRECT7 else 1) and cnt.min() == 0
        g = device(tgt, pts, search=search, **prm)
        o.set_source(pts)
        so, _, _, Po = o.derivatives(p0, eye, True)
        sg, _, _, Pg = g.computeDerivatives(p0, eye, True)
        assert Pg == Po == int(cnt.sum()), (leaf, search)
        assert abs(sg - so) <= 1e-9 * abs(so)
        for i in range(len(pts)):
            g.setInputSource(pts[i:i + 1])
            o.set_source(pts[i:i + 1])
            s1, _, _, P1 = g.computeDerivatives(p0, eye, False)
            assert P1 == int(cnt[i]), (leaf, search, i, pts[i].tolist(), P1, int(cnt[i]))
            if cnt[i]:
                s0 = o.derivatives(p0, eye, False)[0]
                assert abs(s1 - s0) <= 1e-9 * abs(s0), (leaf, search, i, pts[i].tolist())
        g.close()
        o.close()
        rec = both_chains(oracle, tgt, pts, eye, f"faces, leaf {leaf}, search {search}", search=search, **prm)
        assert rec["hist"][0]["pairs"] == int(cnt.sum())


@pytest.mark.parametrize("search,leaf", [(xa.DIRECT1, 0.5), (xa.DIRECT26, 0.5), (xa.DIRECT26, 1.0), (xa.DIRECT1, 1.3),
                                         (xa.DIRECT26, 0.7)])
def test_kernel_variants(oracle, search, leaf):
    """DIRECT1 and DIRECT26 (the multi-tile leading-tail kernel); DIRECT7 is every other test's."""
    pair = scene(seed=7, n_source=1500, leaf=leaf)
    prm = dict(resolution=leaf, step_size=0.1, trans_eps=0.0, max_iter=5, search=search)
    both_chains(oracle, pair.target, pair.source, pair.guess, f"search {search}, leaf {leaf}", **prm)


def test_large_source_tile_loop(oracle):
    """200 000 source points: k_pass_lead<DIRECT7, multi-tile> and its tile loop."""
    pair = small_pair(seed=5, half=60.0, n_source=200_000, max_range=40.0)
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=0.0, max_iter=3, search=xa.DIRECT7)
    g = device(pair.target, pair.source, **prm)
    geom = g.pass_geometry(1)
    assert not geom["one_tile"] and geom["tiles"] > 1
    rec = record(g, pair.guess)
    g.close()
    assert_oracle(oracle, pair.target, pair.source, pair.guess, rec, "200 k source", **prm)


def test_header_change_between_aligns(oracle):
    """Target A (leaf 1.0, dense grid), then target B (leaf 0.5, another box, hash grid) on one context: B's align
    equals a fresh context's bit for bit — no header value survives a build."""
    pa, pb = scene(seed=3), scene(seed=11, leaf=0.5)
    tgt_b = two_clusters(pb, 0.5) + np.array([13.0, -7.0, 2.0], np.float32)
    src_b = pb.source
    guess_b = pb.guess.copy()
    guess_b[:3, 3] += [13.0, -7.0, 2.0]
    prm = dict(step_size=0.1, trans_eps=0.0, max_iter=5, search=xa.DIRECT7)
    for lead in (True, False):
        g = device(pa.target, pa.source, lead, resolution=1.0, **prm)
        ra = record(g, pa.guess)
        assert ra["hist"][0]["pairs"] > 0
        g.setResolution(0.5)
        g.setInputTarget(tgt_b)
        g.setInputSource(src_b)
        rb = record(g, guess_b)
        d = g.grid_info()["div_b"]
        assert d[0] * d[1] * d[2] > GRID_ALLOC_CELLS
        g.close()
        f = device(tgt_b, src_b, lead, resolution=0.5, **prm)
        rf = record(f, guess_b)
        f.close()
        assert rb["hist"][0]["pairs"] > 0
        assert_bitwise(rb, rf, f"second target, lead_tail {lead}")
        # and the other way round: back to A on a context that last ran B
        g2 = device(tgt_b, src_b, lead, resolution=0.5, **prm)
        record(g2, guess_b)
        g2.setResolution(1.0)
        g2.setInputTarget(pa.target)
        g2.setInputSource(pa.source)
        assert_bitwise(record(g2, pa.guess), ra, f"back to the first target, lead_tail {lead}")
        g2.close()
    assert_oracle(oracle, tgt_b, src_b, guess_b, rb, "second target", resolution=0.5, **prm)
