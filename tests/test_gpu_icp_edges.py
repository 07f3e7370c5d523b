"""k_icp_pass at the edges tests/test_gpu_icp.py leaves unrun: ties (the `v == d` branch of NnArg::take, the (d, orig)
order of NnArg::team, the index's fifth word), degenerate targets and queries on every side of the grid, inexact and
doubled index cells, sources past one trip of the grid-stride loop, the estimate's reflection and rank-deficient
branches, ABS_MSE / REL_MSE on the device, and map-frame coordinates.

Reference: tests/icp_restate.py.  Wherever ties are possible it is the brute force over every pair (`exact=True`), with
an identity guess so no f32 transform precedes the search; elsewhere the kd-tree path with the no-ties input condition
of test_gpu_icp.check_first_iteration.  Every input condition is asserted on the reference alone before the device
runs (the same builders are checked without a GPU in tests/test_icp_restate.py).
"""
import numpy as np
import pytest

import icp_edge_scenes as S
import icp_restate as R
from helpers import TF_TOL, small_pair
from test_gpu_icp import PGO, check_first_iteration, make_icp
from test_icp_restate import sparse_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    pair = small_pair(seed=3, n_source=4200)
    src_map = R.transform_f32(pair.guess.astype(np.float32), pair.source)
    rng = np.random.default_rng(12)
    tgt8k = np.ascontiguousarray(pair.target[rng.permutation(len(pair.target))[:8000], :3])
    return {"pair": pair, "tgt": R.Target(pair.target), "src_map": src_map, "tgt8k": tgt8k, "tree8k": R.Target(tgt8k)}


def check_exact(icp, h):
    """The device's last pass against a restatement record, ties allowed: match, d2 bits, pairs exact; mse to 1e-12."""
    idx, d2 = icp.correspondences()
    assert np.array_equal(idx, h["index"]), np.flatnonzero(idx != h["index"])[:10]
    assert np.array_equal(d2.view(np.uint32), h["d2"].view(np.uint32))
    dev = icp.history()
    assert dev[-1]["pairs"] == h["pairs"]
    assert abs(dev[-1]["mse"] - h["mse"]) <= 1e-12 * h["mse"]
    return dev


def run_one_exact(target, source, resolution=1.0):
    """One iteration, identity guess, against the brute force.  Returns the reference's first record."""
    import xchu_slam_amd as xa
    ref = R.icp(source, target, max_iter=1, exact=True)
    h = ref["history"][0]
    assert h["pairs"] == len(source)
    with make_icp(xa, target, source, resolution=resolution, max_iter=1) as icp:
        icp.align(want_output=False)
        check_exact(icp, h)
        assert icp.getFinalNumIteration() == 1 and icp.getConvergenceState() == R.ITERATIONS
    return h


# ---------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("spacing", [1, 2])
@pytest.mark.parametrize("order", ["caller", "reversed"])
def test_ties_lattice(order, spacing):
    """Cell centres (8 candidates in 8 cells), edge midpoints (2), lattice points with repeated target points (d2 = 0,
    ties inside one cell, which the index's stable sort keeps in the caller's order): the winner is the lowest index in
    the caller's order, whichever order that is.  Spacing 1 leaves every tie between cells to NnArg::team; spacing 2 puts
    two candidates of a centre query into one lane's cells, in both cubes (icp_edge_scenes.lattice_scene)."""
    tgt, q, kinds = S.lattice_scene(spacing=spacing)
    census = S.tie_census(q, tgt, 1.0)
    assert census["geo"]["doublings"] == 0
    assert census["tied"].sum() >= 1000, census["tied"].sum()
    assert census["not_first"].sum() >= 100, census["not_first"].sum()
    assert (census["tied"] & (kinds == 2)).sum() >= 100  # in-cell ties of repeated points
    if order == "reversed":
        rev = np.ascontiguousarray(tgt[::-1])
        h = run_one_exact(rev, q)
        # the winners follow the caller's order: most tied queries now pick another point of the target
        moved = (len(tgt) - 1 - h["index"]) != census["winner"]
        assert np.array_equal(moved, census["tied"])
    else:
        h = run_one_exact(tgt, q)
        assert np.array_equal(h["index"], census["winner"])


@pytest.mark.parametrize("resolution", [1.0, 0.5])
def test_ties_block_shells(resolution):
    """Sparse lattice (icp_edge_scenes.sparse_tie_scene): the x-midpoint queries have both equidistant neighbours beyond
    the radius-2 cube and in different 8^3 blocks, so the tie is met and resolved in the block-shell phase."""
    tgt, q, is_x = S.sparse_tie_scene()
    geo = S.index_geometry(tgt, resolution)
    at = S.at_minimum(q, tgt)
    assert np.all(at.sum(1) == 2)
    ct, _ = S.cells_of(tgt, geo)
    cq, _ = S.cells_of(q, geo)
    pair = np.stack([np.flatnonzero(r) for r in at])  # the two candidates of every query
    off = np.abs(ct[pair] - cq[:, None, :]).max(2)     # Chebyshev cell offset of each candidate
    assert np.all(off[is_x] > 2)
    assert np.all(np.any((ct[pair[:, 0]] >> 3) != (ct[pair[:, 1]] >> 3), 1)[is_x])
    if resolution == 1.0:
        assert np.all(off[~is_x].min(1) <= 2) and np.all(off[~is_x].max(1) > 2)  # one inside the cube, one outside
    census = S.tie_census(q, tgt, resolution)
    assert census["not_first"][is_x].sum() >= 20
    run_one_exact(tgt, q, resolution)


# ---------------------------------------------------------------------------------------------- target shapes
@pytest.mark.parametrize("shape", ["one_point", "copies", "one_cell", "one_layer"])
def test_target_shapes(shape):
    """One target point, 500 copies of it, a target inside one cell, a target one cell thick; queries inside the grid
    and 1, 2, 3 and 20 cells outside it on all six sides (c >> 3 on negative cells in the block-shell phase)."""
    tgt = S.shape_targets()[shape]
    q, c, r0, geo = S.queries_around(tgt, 1.0)
    assert geo["doublings"] == 0
    if shape in ("one_point", "copies", "one_cell"):
        assert np.all(geo["div_b"] == 1)
    else:
        assert geo["div_b"][2] == 1 and geo["div_b"][0] > 8 and geo["div_b"][1] > 8
    for axis in range(3):  # every side at every offset, the negative sides included
        for off in (1, 2, 3, 20):
            assert np.any(c[:, axis] == -off) and np.any(c[:, axis] == geo["div_b"][axis] - 1 + off)
    assert np.any(r0 == 0) and np.any((r0 > 0) & (r0 <= 2)) and np.any(r0 > 2)
    h = run_one_exact(tgt, q)
    if shape == "copies":
        assert np.all(h["index"] == 0)


# ---------------------------------------------------------------------------------------------- index cell sizes
@pytest.mark.parametrize("resolution", [0.3, 0.7])
def test_inexact_cell(scene, resolution):
    """small_pair at cell sizes whose f32 reciprocal is inexact."""
    import xchu_slam_amd as xa
    pair, src = scene["pair"], scene["src_map"][:2000]
    cell = np.float32(resolution)
    assert np.float64(np.float32(1.0) / cell) * np.float64(cell) != 1.0  # inv_leaf is a rounded reciprocal
    assert S.index_geometry(pair.target, resolution)["doublings"] == 0
    ref = R.icp(src, pair.target, tgt=scene["tgt"], max_iter=1, k=16)
    with make_icp(xa, pair.target, src, resolution=resolution, max_iter=1) as icp:
        icp.align(want_output=False)
        check_first_iteration(icp, ref)


def test_doubled_cell():
    """Two clusters 400 m apart at resolution 0.1: 369 x 351 x 1 blocks x 512 = 6.6e7 block keys exceed 2^25 = 3.4e7,
    so the index builds at a cell of 0.2 (185 x 176 x 1 blocks, 1.7e7 keys).  The C-ABI does not expose the index cell;
    the doubling is asserted from the build's arithmetic (icp_edge_scenes.index_geometry)."""
    import xchu_slam_amd as xa
    tgt, src = S.doubled_cell_scene()
    geo = S.index_geometry(tgt, 0.1)
    assert geo["doublings"] == 1 and geo["keys"][0] > 1 << 25 >= geo["keys"][1], geo
    assert geo["nbk"][2] == 1 and geo["cell"] == np.float32(0.1) * np.float32(2.0)
    ref = R.icp(src, tgt, max_iter=1, k=16)
    with make_icp(xa, tgt, src, resolution=0.1, max_iter=1) as icp:
        icp.align(want_output=False)
        check_first_iteration(icp, ref)


# ---------------------------------------------------------------------------------------------- grid-stride
def big_source(scene, n, seed=13):
    rng = np.random.default_rng(seed)
    t = scene["tgt8k"]
    return (t[rng.integers(0, len(t), n)].astype(np.float64) + rng.normal(0.0, 0.15, (n, 3))).astype(np.float32)


@pytest.mark.parametrize("n_source", [16384, 16385, 33000])
def test_grid_stride(scene, n_source):
    """16 384 points fill 1024 workgroups x 16 teams once; one more point, and 33 000, take a second and third trip of
    the grid-stride loop."""
    import xchu_slam_amd as xa
    src = big_source(scene, n_source)
    ref = R.icp(src, scene["tgt8k"], tgt=scene["tree8k"], max_iter=1)
    with make_icp(xa, scene["tgt8k"], src, max_iter=1) as icp:
        icp.align(want_output=False)
        dev = check_first_iteration(icp, ref)
        assert dev[0]["pairs"] == n_source
        assert np.max(np.abs(dev[0]["T"] - ref["history"][0]["T"])) < TF_TOL
        assert np.max(np.abs(icp.getFinalTransformation() - ref["final"])) < TF_TOL


def test_grid_stride_second_pass(scene):
    """33 000 points, a non-identity guess, two iterations: the in-place X[i] = p of both passes runs on every trip."""
    import xchu_slam_amd as xa
    src = big_source(scene, 33000)
    guess = S.rigid(0.1, -0.05, 0.02, 0.4).astype(np.float32)
    ref = R.icp(src, scene["tgt8k"], guess, tgt=scene["tree8k"], max_iter=2)
    assert len(ref["history"]) == 2 and not ref["history"][1]["ties"].any()
    with make_icp(xa, scene["tgt8k"], src, max_iter=2) as icp:
        out = icp.align(guess)
        dev = icp.history()
        assert [h["pairs"] for h in dev] == [h["pairs"] for h in ref["history"]] == [33000, 33000]
        for a, b in zip(dev, ref["history"]):
            assert np.max(np.abs(a["T"] - b["T"])) < TF_TOL
        assert np.max(np.abs(icp.getFinalTransformation() - ref["final"])) < TF_TOL
        assert np.array_equal(out, R.transform_f32(icp.getFinalTransformation(), src))
        # the second pass against what it must have seen: X moved by the guess and by the device's own first estimate
        X1 = R.transform_f32(dev[0]["T"], R.transform_f32(guess, src))
        idx, d2, ties = R.correspondences(X1, scene["tree8k"])
        assert not ties.any()
        got_idx, got_d2 = icp.correspondences()
        assert np.array_equal(got_idx, idx) and np.array_equal(got_d2.view(np.uint32), d2.view(np.uint32))
        mse = float(d2.astype(np.float64).sum() / len(d2))
        assert abs(dev[1]["mse"] - mse) <= 1e-12 * mse


# ---------------------------------------------------------------------------------------------- estimates
def run_partner(tgt, src, partners=True, **prm):
    """Align a sparse partner scene (identity guess); the restatement is the brute force.  Input condition (partners):
    the nearest neighbour of every source point is its constructed partner.  Returns (reference, device result, device
    history)."""
    import xchu_slam_amd as xa
    ref = R.icp(src, tgt, exact=True, **prm)
    if partners:
        partner = np.zeros(len(src), int) if len(tgt) == 1 else np.arange(len(src))
        assert np.array_equal(ref["history"][0]["index"], partner)
    with make_icp(xa, tgt, src, **prm) as icp:
        icp.align(want_output=False)
        if len(ref["history"]) == 1:
            check_exact(icp, ref["history"][0])
        return ref, icp.result(), icp.history()


def test_estimate_reflection():
    """Near-planar clouds with independent 1e-3 m z noise on both sides, the seed chosen so det(sigma) < 0: the sign
    of Umeyama's diag(1, 1, s) must be -1, or the estimate is a reflection."""
    tgt, src, seed = S.reflection_scene()
    ref, r, dev = run_partner(tgt, src, max_iter=1)
    assert np.linalg.det(S.sigma_of(src, tgt[ref["history"][0]["index"]])) < 0
    Rd = r["final_tf"][:3, :3].astype(np.float64)
    assert np.linalg.det(Rd) > 0
    assert np.max(np.abs(dev[0]["T"] - ref["history"][0]["T"])) < TF_TOL
    assert np.max(np.abs(r["final_tf"] - ref["final"])) < TF_TOL


def test_estimate_rank2():
    """z exactly 0 on both sides: the cross-covariance has a zero row and column, the rotation is still unique."""
    tgt, src = S.planar_partner_scene(seed=5, z_noise=0.0)
    ref, r, dev = run_partner(tgt, src, max_iter=1)
    assert np.linalg.matrix_rank(S.sigma_of(src, tgt)) == 2
    assert np.linalg.det(r["final_tf"][:3, :3].astype(np.float64)) > 0
    assert np.max(np.abs(dev[0]["T"] - ref["history"][0]["T"])) < TF_TOL


@pytest.mark.parametrize("rank", [1, 0])
def test_estimate_rank_1_and_0(rank):
    """Collinear partners (rank 1) and one target point (rank 0): R is not unique, so its entries are not compared.  It
    must be a rotation, and T must fit the pairs as well as the restatement's does: the root mean squared residual over
    the first iteration's pairs within sqrt(3) * delta, delta = 4 * 2^-23 * max|p| + ulp32(max|t|) (one f32 ulp in each
    entry of T moves a coordinate by at most delta)."""
    tgt, src = S.collinear_scene() if rank == 1 else S.one_target_scene()
    ref, r, dev = run_partner(tgt, src, max_iter=1)
    h = ref["history"][0]
    Q = tgt[h["index"]]
    assert np.linalg.matrix_rank(S.sigma_of(src, Q), tol=1e-9) == rank
    assert (r["state"], r["n_pairs"], r["nr_iterations"]) == (ref["state"], ref["pairs"], 1)
    Rd = r["final_tf"][:3, :3].astype(np.float64)
    assert np.max(np.abs(Rd.T @ Rd - np.eye(3))) <= 1e-6
    assert np.linalg.det(Rd) > 0
    delta = S.residual_delta(src, h["T"])
    got, want = S.residual_rms(r["final_tf"], src, Q), S.residual_rms(h["T"], src, Q)
    print("rank", rank, "residual rms", got, "restatement", want, "bar", np.sqrt(3) * delta)
    assert abs(got - want) <= np.sqrt(3) * delta


def test_exact_subset(scene):
    """Source = the first 200 target points, identity guess: every d2 is 0 and the estimate is the identity."""
    import xchu_slam_amd as xa
    tgt, src = scene["tgt8k"], scene["tgt8k"][:200]
    ref = R.icp(src, tgt, tgt=scene["tree8k"], trans_eps=1e-6)
    assert (ref["state"], ref["iterations"]) == (R.TRANSFORM, 1)
    with make_icp(xa, tgt, src, trans_eps=1e-6) as icp:
        icp.align(want_output=False)
        r = icp.result()
        assert (r["state"], r["nr_iterations"], r["converged"], r["mse"]) == (R.TRANSFORM, 1, True, 0.0)
    ref = R.icp(src, tgt, tgt=scene["tree8k"], trans_eps=0.0, fit_eps=0.0)
    assert [h["state"] for h in ref["history"]] == [R.NOT_CONVERGED, R.ABS_MSE]
    with make_icp(xa, tgt, src, trans_eps=0.0, fit_eps=0.0) as icp:
        icp.align(want_output=False)
        dev = icp.history()
        assert [h["state"] for h in dev] == [R.NOT_CONVERGED, R.ABS_MSE]
        assert [h["mse"] for h in dev] == [0.0, 0.0] and [h["pairs"] for h in dev] == [200, 200]
        assert icp.hasConverged() and icp.getFinalNumIteration() == 2


@pytest.mark.parametrize("case", ["abs_mse", "rel_mse"])
def test_mse_states(case):
    """The two constructed cases of tests/test_icp_restate.py on the device: ABS_MSE (both epsilons off, the mse settles
    at the f32 rounding floor; the first comparison is against prev = DBL_MAX) and REL_MSE (a noisy target,
    fit_eps = 0.5).  The 300-point targets put nearly every query in the block-shell phase.  The cases are taken as they
    are: in the second, 3 of the 200 source points have a nearer neighbour than their partner, so the partner condition
    is asserted for the first only."""
    if case == "abs_mse":
        tgt, src, _ = sparse_scene()
        prm, last = dict(max_iter=50), R.ABS_MSE
    else:
        tgt, src, _ = sparse_scene(seed=1)
        tgt = (tgt + np.random.default_rng(5).normal(0, 0.05, tgt.shape)).astype(np.float32)
        prm, last = dict(max_iter=50, fit_eps=0.5), R.REL_MSE
    ref, r, dev = run_partner(tgt, src, partners=case == "abs_mse", **prm)
    assert ref["state"] == last and ref["iterations"] >= 2
    assert (r["state"], r["nr_iterations"], r["converged"]) == (ref["state"], ref["iterations"], True)
    assert [h["state"] for h in dev] == [h["state"] for h in ref["history"]]
    assert [h["pairs"] for h in dev] == [h["pairs"] for h in ref["history"]]


# ---------------------------------------------------------------------------------------------- map frame
@pytest.fixture(scope="module")
def map_scene(scene):
    """small_pair moved to a map-frame position: shifted on the host in f64, rounded to f32 once."""
    tgt = (scene["pair"].target[:, :3].astype(np.float64) + S.MAP_OFFSET).astype(np.float32)
    src = (scene["src_map"][:3000].astype(np.float64) + S.MAP_OFFSET).astype(np.float32)
    return {"target": tgt, "source": src, "tgt": R.Target(tgt)}


def test_map_frame_first_iteration(map_scene):
    """At |q| ~ 640 m the 4e-7 |q| part of the walk's slack exceeds the 1e-4 cell part, and the estimate subtracts
    n q p^T from uncentred f64 sums: matches and d2 exact, every entry of T within one f32 spacing of the restatement's
    (measured on the MI355X: no entry differs)."""
    import xchu_slam_amd as xa
    tgt, src = map_scene["target"], map_scene["source"]
    assert 4e-7 * np.abs(src).sum(1).min() > 1e-4 * 1.0
    ref = R.icp(src, tgt, tgt=map_scene["tgt"], max_iter=1)
    with make_icp(xa, tgt, src, max_iter=1) as icp:
        icp.align(want_output=False)
        dev = check_first_iteration(icp, ref)
        Tr = ref["history"][0]["T"]
        print("map frame, one iteration: entries of T that differ", int((dev[0]["T"] != Tr).sum()), "worst",
              float(np.max(np.abs(dev[0]["T"].astype(np.float64) - Tr.astype(np.float64)))))
        assert np.all(np.abs(dev[0]["T"].astype(np.float64) - Tr.astype(np.float64)) <= np.spacing(np.abs(Tr)).astype(np.float64))


def test_map_frame_full_align(map_scene):
    """pgo_node's settings at the map-frame position: iteration count, final state and per-iteration pair counts equal
    the restatement's.  The bar for `final` is ten times the spread of the restatement's own `final` between umeyama in
    f64 and in np.longdouble, and at least one f32 ulp of the largest entry of `final`.
    Measured (MI355X; DESIGN.md section 2, ICP): 26 iterations, REL_MSE on both sides (the origin-centred scene takes 21
    and ends in TRANSFORM: at |q| ~ 640 m the f32 coordinates are 64 times coarser); spread 0.0 (the two restatement
    runs are bit-equal in every f32 transform), so the bar is the ulp floor, 9.54e-7 (largest entry 9.42); device
    difference 0.0."""
    import xchu_slam_amd as xa
    tgt, src = map_scene["target"], map_scene["source"]
    ref = R.icp(src, tgt, tgt=map_scene["tgt"], **PGO)
    ref_ld = R.icp(src, tgt, tgt=map_scene["tgt"], estimate_dtype=np.longdouble, **PGO)
    spread = float(np.max(np.abs(ref["final"].astype(np.float64) - ref_ld["final"].astype(np.float64))))
    bar = max(10.0 * spread, S.ulp32(np.max(np.abs(ref["final"]))))
    with make_icp(xa, tgt, src, **PGO) as icp:
        icp.align(want_output=False)
        r, dev = icp.result(), icp.history()
        diff = float(np.max(np.abs(r["final_tf"].astype(np.float64) - ref["final"].astype(np.float64))))
        print("iterations", r["nr_iterations"], R.STATE_NAMES[r["state"]], "spread", spread, "bar", bar, "device", diff)
        assert (r["nr_iterations"], r["state"], r["converged"]) == (ref["iterations"], ref["state"], ref["converged"])
        assert [h["pairs"] for h in dev] == [h["pairs"] for h in ref["history"]]
        assert diff <= bar
