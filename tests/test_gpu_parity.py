"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle on identical seeded inputs.

Bars:
  * voxel grid: integer work (keys, point counts, rejection flags, cloud order) bit-exact; f64 means bit-exact;
    f64 inverse covariances within 1e-12 relative (same Eigen-3.3 algorithm, host vs device libm).
  * one derivative pass at a fixed (p, T): pair count P bit-exact; score / gradient / Hessian within 1e-9
    relative against the oracle, which evaluates every per-pair f32 term as the shipped libndt_omp.so does
    ((float)exp((double)x), Eigen's SSE reduction orders; tests/native/libm_check.cpp and sse_order_check.cpp: the
    device's per-pair f32 terms are the same bits, only the f64 summation order differs); glibc's expf instead (oracle
    exp_mode 0, not what the binary calls) differs by one f32 ulp on ~0.4 % of pairs (within 2e-6).
  * full align: every per-iteration parameter vector within X_TOL = 1e-12 (north star: 1e-4 m / 1e-4 rad; measured
    <= 3e-15, tools/parity_margins.py), the same pair count in every pass, final f32 transform within TF_TOL = 1e-6
    (measured bit-equal), identical iteration counts and convergence flags.
"""
import numpy as np
import pytest

from helpers import TF_TOL, X_TOL, f32_transform, pose_err, rel_err, small_pair

pytestmark = pytest.mark.gpu

xa = pytest.importorskip("xchu_slam_amd")


def make_pair_objs(oracle, pair, exp_mode=1, **prm):
    o = oracle.OracleNDT(num_threads=1, exp_mode=exp_mode, **prm)
    o.set_target(pair.target)
    o.set_source(pair.source)
    g = xa.NormalDistributionsTransform()
    for k, v in prm.items():
        setattr(g._params, k, v)
    g._push()
    g.setInputTarget(pair.target)
    g.setInputSource(pair.source)
    return o, g


def test_grid_bit_exact(oracle):
    pair = small_pair()
    o, g = make_pair_objs(oracle, pair, resolution=1.0)
    oh, gh = o.grid_header(), g.grid_info()
    for k in ("min_b", "max_b", "div_b", "divb_mul", "n_leaves", "n_cloud", "overflow"):
        assert oh[k] == gh[k], k
    ol, gl = o.grid_leaves(), g.grid_leaves()
    cloud = ol["npts"] != 0
    # oracle exports every leaf (ascending key); the device keeps the KD cloud (>= min points, ascending key)
    sel = (ol["npts"] >= 6) | (ol["npts"] == -1)
    assert np.array_equal(ol["keys"][sel], gl["keys"])
    assert np.array_equal(ol["npts"][sel], gl["npts"])
    assert np.array_equal(ol["mean"][sel], gl["mean"])
    assert np.array_equal(ol["centroid"][sel], gl["centroid"])
    valid = gl["npts"] > 0
    assert rel_err(gl["icov"][valid], ol["icov"][sel][valid]) < 1e-12
    assert cloud.sum() >= sel.sum()


def grid_matches(oracle_obj, g):
    oh, gh = oracle_obj.grid_header(), g.grid_info()
    for k in ("min_b", "max_b", "div_b", "divb_mul", "n_leaves", "n_cloud", "overflow"):
        assert oh[k] == gh[k], k
    ol, gl = oracle_obj.grid_leaves(), g.grid_leaves()
    sel = (ol["npts"] >= 6) | (ol["npts"] == -1)
    for k in ("keys", "npts", "mean", "centroid"):
        assert np.array_equal(ol[k][sel], gl[k]), k
    valid = gl["npts"] > 0
    assert rel_err(gl["icov"][valid], ol["icov"][sel][valid]) < 1e-12
    return gl


def test_grid_rebuild_and_non_dense(oracle):
    """Rebuilding the same target in a ctx (grid already sized, buffers reused) gives the same grid bit for
    bit; a non-dense target's non-finite points are skipped (voxel_grid_covariance_omp_impl.hpp:207-213)."""
    pair = small_pair()
    o, g = make_pair_objs(oracle, pair, resolution=1.0)
    first = grid_matches(o, g)
    g.setInputTarget(pair.target)
    second = grid_matches(o, g)
    for k in ("keys", "npts", "mean", "icov", "centroid"):
        assert np.array_equal(first[k], second[k]), k
    # non-finite points of a non-dense cloud are skipped by both paths
    tgt = pair.target.copy()
    tgt[::97] = np.nan
    o2 = oracle.OracleNDT(num_threads=1, resolution=1.0)
    o2.set_target(tgt, is_dense=False)
    g.setInputTarget(tgt, is_dense=False)
    grid_matches(o2, g)


def test_grid_long_and_boundary_runs(oracle):
    """Voxel runs of the sorted keys that cross 4096-key tiles and leave the 64-key halo of the fused segment /
    cloud scan (one voxel of 30 000 points, several of 5 000), next to voxels of exactly min_points and
    min_points - 1 points: same segments, cloud voxels and moments as the oracle."""
    rng = np.random.default_rng(21)
    parts = [rng.uniform(0.05, 0.95, (30_000, 3)) + [2.0, 3.0, 1.0]]
    for k in range(6):
        parts.append(rng.uniform(0.05, 0.95, (5_000, 3)) + [5.0 + k, 1.0, 2.0])
    for k in range(200):
        n = 6 if k % 2 == 0 else 5  # exactly min_points / one short of it
        parts.append(rng.uniform(0.05, 0.95, (n, 3)) + [float(k % 20), 8.0 + k // 20, 0.0])
    parts.append(rng.uniform(0.0, 20.0, (20_000, 3)))
    tgt = np.concatenate(parts).astype(np.float32)[rng.permutation(sum(len(p) for p in parts))]
    o = oracle.OracleNDT(num_threads=1, resolution=1.0)
    o.set_target(tgt)
    g = xa.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setInputTarget(tgt)
    gl = grid_matches(o, g)
    assert gl["npts"].max() >= 30_000


@pytest.mark.parametrize("n_vox", [4096, 8192, 4095])
def test_grid_one_point_per_voxel(oracle, n_vox):
    """Every target point in a voxel of its own, min_points_per_voxel = 1 (setMinPointPerVoxel keeps 3 as its floor, so
    the ctx parameter is set directly): n_leaves == M, a multiple of the 4096-key scan tile — the cloud scan's last tile
    must still publish n_cloud (it was taken from the tile past the grid)."""
    rng = np.random.default_rng(5)
    side = int(np.ceil(n_vox ** (1 / 3))) + 1
    cells = rng.permutation(side ** 3)[:n_vox]
    ijk = np.stack([cells % side, (cells // side) % side, cells // (side * side)], 1).astype(np.float32)
    tgt = (ijk + rng.uniform(0.2, 0.8, ijk.shape)).astype(np.float32)
    o = oracle.OracleNDT(num_threads=1, resolution=1.0, min_points_per_voxel=1)
    o.set_target(tgt)
    g = xa.NormalDistributionsTransform()
    g._params.resolution = 1.0
    g._params.min_points_per_voxel = 1
    g._push()
    g.setInputTarget(tgt)
    oh, gh = o.grid_header(), g.grid_info()
    assert gh["n_leaves"] == n_vox and gh["n_cloud"] == n_vox
    for k in ("min_b", "max_b", "div_b", "n_leaves", "n_cloud"):
        assert oh[k] == gh[k], k
    gl, ol = g.grid_leaves(), o.grid_leaves()
    assert np.array_equal(ol["keys"], gl["keys"])
    assert np.array_equal(ol["mean"], gl["mean"])


def test_large_extent_hash_grid(oracle):
    """A map whose bounding box exceeds the dense cell grid allocation (~19.8 M cells > 16 M) is looked up
    through the open-addressing hash instead: same grid and same align as the oracle; a later build of a
    small map switches back to the dense grid."""
    pair = small_pair()
    far = np.array([[-150.0, -150.0, -20.0], [150.0, 150.0, 230.0]], np.float32)  # ~19.8 M cells > 16 M
    big = np.concatenate([pair.target, far]).astype(np.float32)
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=0.0, max_iter=10)
    o = oracle.OracleNDT(num_threads=1, **prm)
    o.set_target(big)
    o.set_source(pair.source)
    g = xa.NormalDistributionsTransform()
    for k, v in prm.items():
        setattr(g._params, k, v)
    g._push()
    g.setInputTarget(pair.target)      # dense grid (16 M cells allocated)
    g.setInputSource(pair.source)
    g.align(pair.guess, want_output=False)
    g.setInputTarget(big)              # bbox too large for the allocation: hash lookup
    g.align(pair.guess, want_output=False)
    rg, ro = g.result(), o.align(pair.guess)
    assert rg["nr_iterations"] == ro["nr_iterations"]
    assert np.max(np.abs(rg["final_tf"] - ro["final_tf"])) < TF_TOL
    grid_matches(o, g)
    o_small = oracle.OracleNDT(num_threads=1, resolution=1.0)
    o_small.set_target(pair.target)
    g.setInputTarget(pair.target)
    grid_matches(o_small, g)


@pytest.mark.parametrize("search", [2, 1, 3, 0])
def test_single_pass(oracle, search):
    pair = small_pair()
    o, g = make_pair_objs(oracle, pair, resolution=1.0, search=search)
    p = oracle.initial_p(pair.guess)
    T = pair.guess.astype(np.float32)
    so, go, Ho, Po = o.derivatives(p, T, True)
    sg, gg, Hg, Pg = g.computeDerivatives(p, T, True)
    assert Po == Pg and Po > 0
    assert abs(so - sg) <= 1e-9 * abs(so)
    assert rel_err(gg, go) < 1e-9
    assert rel_err(Hg, Ho) < 1e-9
    # against glibc's expf instead of the binary's (float)exp((double)x): what the 1e-9 bar above pins
    o1, _ = make_pair_objs(oracle, pair, exp_mode=0, resolution=1.0, search=search)
    s1, g1, H1, P1 = o1.derivatives(p, T, True)
    assert P1 == Pg
    assert abs(s1 - sg) <= 2e-6 * abs(s1) and rel_err(gg, g1) < 2e-6 and rel_err(Hg, H1) < 2e-6
    # gradient-only pass (MT trial) leaves H at zero
    sg2, gg2, Hg2, _ = g.computeDerivatives(p, T, False)
    assert sg2 == sg and np.array_equal(gg2, gg) and not Hg2.any()


def test_hessian_radius(oracle):
    pair = small_pair()
    o, g = make_pair_objs(oracle, pair, resolution=1.0)
    p = oracle.initial_p(pair.guess)
    T = pair.guess.astype(np.float32)
    Ho, Po = o.hessian_radius(p, T)
    Hg, Pg = g.computeHessianRadius(p, T)
    assert Po == Pg and Po > 0
    assert rel_err(Hg, Ho) < 1e-9


@pytest.mark.parametrize("eps,search,mode", [(0.0, 2, 0), (0.01, 2, 0), (0.01, 1, 0), (0.0, 0, 0), (0.01, 2, 1)])
def test_align_per_iteration(oracle, eps, search, mode):
    pair = small_pair()
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=eps, max_iter=30, search=search, precision_mode=mode)
    o, g = make_pair_objs(oracle, pair, **prm)
    ro = o.align(pair.guess)
    g.align(pair.guess, want_output=False)
    rg = g.result()
    ho, hg = o.history(), g.history()
    assert rg["nr_iterations"] == ro["nr_iterations"]
    assert rg["converged"] == ro["converged"]
    assert len(ho) == len(hg)
    for a, b in zip(ho, hg):
        assert a["kind"] == b["kind"] and a["newton_iter"] == b["newton_iter"]
        assert np.max(np.abs(a["x"] - b["x"])) < X_TOL
        assert a["pairs"] == b["pairs"]
    assert np.max(np.abs(rg["final_tf"] - ro["final_tf"])) < TF_TOL
    assert abs(rg["trans_probability"] - ro["trans_probability"]) <= 1e-6 * abs(ro["trans_probability"]) + 1e-12
    t_err, r_err = pose_err(rg["final_tf"], pair.true_pose)
    assert t_err < 0.2 and r_err < 0.5


@pytest.mark.parametrize("search", [xa.DIRECT7, xa.DIRECT26])
def test_align_records_reevaluated(oracle, search):
    """Every pass the device recorded during align, re-evaluated by the oracle at the device's own x
    (computeDerivatives, ndt_omp_impl.hpp:175-251): the neighbour sets agree exactly and score/g/H to 1e-9.
    The oracle evaluates exp and sin / cos as the binary's model (exp_mode 1, trig_mode 1): the device computes the
    same f32 values (ndt_libm.h), so the transform of every pass is the oracle's own."""
    pair = small_pair()
    o, g = make_pair_objs(oracle, pair, resolution=1.0, step_size=0.1, trans_eps=0.0, max_iter=12, search=search)
    g.align(pair.guess, want_output=False)
    hist = g.history()
    assert len(hist) == 12 + 3
    for i, rec in enumerate(hist):
        x = np.asarray(rec["x"], np.float64)
        # pass 0 runs on the cloud transformed by the guess itself (computeTransformation, ndt_omp_impl.hpp:79-96),
        # every later pass on convertTransform(x_t)
        T = pair.guess.astype(np.float32) if i == 0 else oracle.convert_transform(x)
        hess = rec["kind"] == 0
        so, go, Ho, Po = o.derivatives(x, T, hess)
        assert rec["pairs"] == Po
        assert abs(rec["score"] - so) <= 1e-9 * abs(so)
        assert rel_err(rec["g"], go) < 1e-9
        if hess:
            assert rel_err(rec["H"], Ho) < 1e-9


@pytest.mark.parametrize("res", [1.0, 0.5])
def test_calculate_score(oracle, res):
    """calculateScore (ndt_omp_impl.hpp:919-952): f64 score over the radius neighbours, per-point normalised;
    same neighbour sets and terms as the oracle, summed in a different fixed order (1e-12).  Like the reference,
    it reads the Gaussian constants held by the object: the constructor's (resolution 1.0, :46-63) until an
    align recomputes them for the current resolution (:80-87)."""
    pair = small_pair()
    o, g = make_pair_objs(oracle, pair, resolution=res, trans_eps=0.0, max_iter=5)
    for T in (pair.guess.astype(np.float32), pair.true_pose.astype(np.float32)):
        so, sg = o.calculate_score(T), g.calculateScore(T)
        assert so != 0.0 and abs(sg - so) <= 1e-12 * abs(so)
    g.align(pair.guess, want_output=False)
    o.align(pair.guess)  # both objects now hold the constants of the current resolution
    Tf = g.getFinalTransformation()
    assert abs(g.calculateScore() - o.calculate_score(Tf)) <= 1e-12 * abs(o.calculate_score(Tf))


@pytest.mark.parametrize("res", [1.0, 0.5, 0.05])
def test_fitness_score_vs_kdtree(res):
    """getFitnessScore (pcl::Registration, odom_node.cpp:280): exact nearest neighbour over ALL target points.
    Checked against scipy's cKDTree: every device squared distance (float32, FLANN order) is the float32
    distance to a nearest neighbour; the fitness is their mean; max_range filters squared distances.
    At res 0.05 the index doubles its cell: the 80 m x 80 m x 14.5 m target spans 1601 x 1601 x 291 cells of 0.05 m,
    201 x 201 x 37 blocks of 8^3 cells = 765e6 keys > 2^25; 0.1 m still gives 101 x 101 x 19 x 512 = 99e6, 0.2 m fits
    (51 x 51 x 10 x 512 = 13e6).  The target's voxel grid (1601 x 1601 x 291 = 7.5e8 < 2^31 voxels) does not overflow."""
    from scipy.spatial import cKDTree
    pair = small_pair()

    def shifted(T, d):
        S = np.array(T, np.float64).copy()
        S[:3, 3] += d
        return S.astype(np.float32)

    rng = np.random.default_rng(5)
    sparse = np.asarray(pair.target, np.float32)[rng.random(len(pair.target)) < 0.03]
    # full target, and a sparse one whose neighbours are often several cells away (block-shell phase)
    for tgt_cloud in (pair.target, sparse):
        g = xa.NormalDistributionsTransform()
        g.setResolution(res)
        g.setInputTarget(tgt_cloud)
        g.setInputSource(pair.source)
        tgt = np.asarray(tgt_cloud, np.float32)
        tree = cKDTree(tgt.astype(np.float64))
        # guess / truth, a 27 m offset (most queries far from their neighbour) and one far outside the target box
        for T in (pair.guess, pair.true_pose, shifted(pair.guess, [25.0, -10.0, 4.0]), shifted(pair.guess, [400.0, 0.0, -50.0])):
            f, d2 = g.getFitnessScore(T=T, return_distances=True)
            xt = f32_transform(T, pair.source)
            _, idx = tree.query(xt.astype(np.float64))
            u = tgt[idx] - xt
            ref = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
            assert np.all(d2 <= ref)                              # never worse than the KD tree's neighbour
            assert np.allclose(d2, ref, rtol=2e-6, atol=1e-12)    # same neighbour up to float near-ties
            assert abs(f - float(np.sum(d2.astype(np.float64))) / len(d2)) <= 1e-12 * f
            lim = float(np.median(d2))
            f_lim = g.getFitnessScore(max_range=lim, T=T)
            sel = d2.astype(np.float64) <= lim
            assert abs(f_lim - d2[sel].astype(np.float64).mean()) <= 1e-12 * f_lim
    g.setInputTarget(pair.target)
    assert g.getFitnessScore(max_range=-1.0, T=pair.guess) == np.finfo(np.float64).max
    g.setMaximumIterations(5)
    g.align(pair.guess, want_output=False)
    assert g.getFitnessScore() == g.getFitnessScore(T=g.getFinalTransformation())


@pytest.mark.parametrize("step,eps", [(0.001, 2.0), (0.01, 0.5)])
def test_mt_inner_loop(oracle, step, eps):
    """step_size <= eps/2 lets the More-Thuente inner loop + radius computeHessian run (ndt_omp_impl.hpp:807-913)."""
    pair = small_pair()
    prm = dict(resolution=1.0, step_size=step, trans_eps=eps, max_iter=4)
    o, g = make_pair_objs(oracle, pair, **prm)
    ro = o.align(pair.guess)
    g.align(pair.guess, want_output=False)
    rg = g.result()
    ho, hg = o.history(), g.history()
    assert [h["kind"] for h in ho] == [h["kind"] for h in hg]
    assert any(h["kind"] == 2 for h in ho)
    for a, b in zip(ho, hg):
        assert np.max(np.abs(a["x"] - b["x"])) < X_TOL
    assert rg["nr_iterations"] == ro["nr_iterations"]


def test_output_cloud_and_determinism(oracle):
    pair = small_pair()
    o, g = make_pair_objs(oracle, pair, resolution=1.0, trans_eps=0.0, max_iter=10)
    ro = o.align(pair.guess, want_output=True)
    out1 = g.align(pair.guess)
    h1 = g.history()
    out2 = g.align(pair.guess)
    h2 = g.history()
    assert np.array_equal(out1, out2)
    for a, b in zip(h1, h2):  # bitwise run-to-run determinism
        assert a["score"] == b["score"] and np.array_equal(a["g"], b["g"]) and np.array_equal(a["H"], b["H"])
    assert np.max(np.abs(out1 - ro["output"])) < 1e-4


@pytest.mark.parametrize("search,eps", [(xa.DIRECT7, 0.01), (xa.DIRECT7, 0.0), (xa.KDTREE, 0.01)])
def test_source_sizes_share_chains(oracle, search, eps):
    """Scans of changing size (odom_node's filtered scans) reuse one captured pass chain per size bucket (geom_points:
    the kernels take the real point count from the align state): every align equals a fresh context's align of the same
    cloud bit for bit, and stays within the usual bars of the oracle."""
    pair = small_pair()
    src = np.asarray(pair.source, np.float32)
    sizes = [len(src) - 13 * k for k in (0, 3, 1, 5, 2, 0)]
    g = xa.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setTransformationEpsilon(eps)
    g.setMaximumIterations(8)
    g.setNeighborhoodSearchMethod(search)
    g.setInputTarget(pair.target)
    for n in sizes:
        g.setInputSource(src[:n])
        g.align(pair.guess, want_output=False)
        r, h = g.result(), g.history()
        f = xa.NormalDistributionsTransform()
        f.setResolution(1.0)
        f.setTransformationEpsilon(eps)
        f.setMaximumIterations(8)
        f.setNeighborhoodSearchMethod(search)
        f.setInputTarget(pair.target)
        f.setInputSource(src[:n])
        f.align(pair.guess, want_output=False)
        rf, hf = f.result(), f.history()
        f.close()
        assert np.array_equal(r["final_tf"], rf["final_tf"]) and r["nr_iterations"] == rf["nr_iterations"], n
        assert len(h) == len(hf)
        for a, b in zip(h, hf):
            assert a["score"] == b["score"] and a["pairs"] == b["pairs"] and np.array_equal(a["H"], b["H"]), n
        o = oracle.OracleNDT(num_threads=1, resolution=1.0, trans_eps=eps, max_iter=8, search=search)
        o.set_target(pair.target)
        o.set_source(src[:n])
        ro = o.align(pair.guess)
        assert r["nr_iterations"] == ro["nr_iterations"], n
        assert np.max(np.abs(r["final_tf"] - ro["final_tf"])) < TF_TOL, n
    g.close()


def test_identity_guess_and_errors(oracle):
    pair = small_pair()
    g = xa.NormalDistributionsTransform()
    with pytest.raises(xa._lib.NdtError) as e:
        g.align(np.eye(4))
    assert e.value.status == xa._lib.NDT_ENOTARGET
    g.setInputTarget(pair.target)
    with pytest.raises(xa._lib.NdtError) as e:
        g.align(np.eye(4))
    assert e.value.status == xa._lib.NDT_ENOSOURCE
    g.setInputSource(pair.source)
    g.setTransformationEpsilon(0.01)
    g.align(np.eye(4), want_output=False)
    o = oracle.OracleNDT(num_threads=1, trans_eps=0.01)
    o.set_target(pair.target)
    o.set_source(pair.source)
    ro = o.align(np.eye(4))
    assert g.getFinalNumIteration() == ro["nr_iterations"]
    assert np.max(np.abs(g.getFinalTransformation() - ro["final_tf"])) < TF_TOL


def test_degenerate_targets(oracle):
    g = xa.NormalDistributionsTransform()
    src = np.random.default_rng(0).normal(0, 1, (500, 3)).astype(np.float32)
    # every target point in one voxel: a single leaf
    tgt = np.random.default_rng(1).uniform(0.1, 0.9, (50, 3)).astype(np.float32)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    g.align(np.eye(4), want_output=False)
    info = g.grid_info()
    assert info["n_leaves"] == 1 and info["n_cloud"] == 1
    o = oracle.OracleNDT(num_threads=1)
    o.set_target(tgt)
    o.set_source(src)
    ro = o.align(np.eye(4))
    assert g.getFinalNumIteration() == ro["nr_iterations"] and g.hasConverged() == bool(ro["converged"])
    # too few points per voxel: empty grid -> zero derivatives -> immediate exit, converged (norm == 0)
    g.setInputTarget(np.array([[0, 0, 0], [5, 5, 5]], np.float32))
    g.align(np.eye(4), want_output=False)
    assert g.hasConverged() and g.getFinalNumIteration() == 0
    # index overflow guard: grid empty
    g.setResolution(1e-3)
    g.setInputTarget(np.array([[0, 0, 0], [1e4, 1e4, 1e4]] * 4, np.float32))
    assert g.grid_info()["overflow"] == 1


def test_downsample(oracle):
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-20, 20, (20000, 3)), rng.uniform(0, 100, (20000, 1))], 1).astype(np.float32)
    ref = oracle.voxel_downsample(pts, 1.0)
    out = xa.voxel_downsample(pts, 1.0)
    assert out.shape == ref.shape
    assert np.array_equal(out, ref)


def test_batch_matches_single(oracle):
    pair = small_pair()
    g = xa.NormalDistributionsTransform()
    g.setTransformationEpsilon(0.0)
    g.setMaximumIterations(10)
    dt = g.device_upload(np.concatenate([pair.target, np.ones((len(pair.target), 1), np.float32)], 1))
    ds = g.device_upload(np.concatenate([pair.source, np.ones((len(pair.source), 1), np.float32)], 1))
    res = g.align_batch([(dt, len(pair.target), ds, len(pair.source), pair.guess)] * 2)
    g.setInputTarget(pair.target)
    g.setInputSource(pair.source)
    g.align(pair.guess, want_output=False)
    single = g.result()
    for r in res:
        assert np.array_equal(r["final_tf"], single["final_tf"])
        assert r["nr_iterations"] == single["nr_iterations"]
    g.device_free(dt)
    g.device_free(ds)


@pytest.mark.parametrize("eps,iters", [(0.0, 6), (0.01, 30)])
def test_batch_many_pairs_matches_single(oracle, eps, iters):
    """ndt_align_batch over 19 distinct pairs (every stream reused several times, fixed-work and converging chains):
    every pair's record is bit for bit the one a single align of that pair gives; a batch with one odd-sized pair too."""
    pairs = [small_pair(seed=40 + k, n_source=3000) for k in range(19)]
    g = xa.NormalDistributionsTransform()
    g.setTransformationEpsilon(eps)
    g.setMaximumIterations(iters)
    dev = []
    for p in pairs:
        dt = g.device_upload(np.concatenate([p.target, np.ones((len(p.target), 1), np.float32)], 1))
        ds = g.device_upload(np.concatenate([p.source, np.ones((len(p.source), 1), np.float32)], 1))
        dev.append((dt, len(p.target), ds, len(p.source), p.guess))
    lock = g.align_batch(dev)
    mixed = g.align_batch(dev[:4] + [(dev[4][0], dev[4][1], dev[4][2], dev[4][3] - 7, dev[4][4])])
    singles = []
    for p in pairs:
        g.setInputTarget(p.target)
        g.setInputSource(p.source)
        g.align(p.guess, want_output=False)
        singles.append(g.result())
    for k, (r, ref) in enumerate(zip(lock, singles)):
        assert np.array_equal(r["final_tf"], ref["final_tf"]), k
        for f in ("nr_iterations", "converged", "n_passes", "n_pairs", "score", "trans_probability"):
            assert r[f] == ref[f], (k, f, r[f], ref[f])
    for k in range(4):
        assert np.array_equal(mixed[k]["final_tf"], singles[k]["final_tf"]), k
    for d in dev:
        g.device_free(d[0])
        g.device_free(d[2])
    g.close()


def test_align_source_order(oracle):
    """Clouds of >= 262144 points are visited in target-cell order during an align (k_src_keys): the same
    per-point arithmetic in a different f64 summation order.  Against the oracle: identical pair counts and
    iteration path within 1e-6; against the device run in caller order: per-pass results within 1e-9."""
    pair = small_pair(seed=5, half=60.0, n_source=280000, max_range=40.0)
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=0.0, max_iter=12)
    o, g = make_pair_objs(oracle, pair, **prm)
    ro = o.align(pair.guess)
    g.align(pair.guess, want_output=False)
    rg, hg, ho = g.result(), g.history(), o.history()
    assert rg["nr_iterations"] == ro["nr_iterations"] and len(hg) == len(ho)
    # every pass runs at the oracle's transform to f64 rounding: the same pairs exactly
    assert ho[0]["pairs"] == hg[0]["pairs"]
    for a, b in zip(ho, hg):
        assert a["pairs"] == b["pairs"]
        assert np.max(np.abs(a["x"] - b["x"])) < X_TOL
    _, g0 = make_pair_objs(oracle, pair, **prm)
    g0.set_pass_options(source_order=False)
    g0.align(pair.guess, want_output=False)
    h0 = g0.history()
    assert len(h0) == len(hg) and h0[0]["pairs"] == hg[0]["pairs"]
    for a, b in zip(h0, hg):
        assert abs(a["pairs"] - b["pairs"]) <= 2
        assert np.max(np.abs(a["x"] - b["x"])) < 1e-9
        assert abs(a["score"] - b["score"]) <= 1e-9 * abs(a["score"])
        assert rel_err(b["H"], a["H"]) < 1e-9
    # the aligned output cloud keeps the caller's point order
    out = g.align(pair.guess)
    ref = (pair.source.astype(np.float32) @ rg["final_tf"][:3, :3].T.astype(np.float32)) + rg["final_tf"][:3, 3]
    assert np.max(np.abs(out - ref)) < 1e-3


def _line_world(rng, n, lo, hi):
    """points exactly on the x axis (y = z = 0): the Newton system loses rank (rotations about x and the cross-axis
    directions carry no information up to rounding)."""
    return np.stack([rng.uniform(lo, hi, n), np.zeros(n), np.zeros(n)], 1).astype(np.float32)


def _corridor(rng, n, half_len=15.0, width=2.37, height=3.0, floor=0.37):
    """two facades y = +-width and an exactly flat floor z = floor: translation along the corridor is constrained only
    by the voxel discretisation (a near-degenerate x direction).  The planes sit inside cells, not on cell faces (a
    point exactly on a face changes cell with the last ulp of the transform, in the reference as here)."""
    k = rng.integers(0, 3, n)
    x = rng.uniform(-half_len, half_len, n)
    y = np.where(k == 0, -width, np.where(k == 1, width, rng.uniform(-width, width, n)))
    z = np.where(k == 2, floor, rng.uniform(floor, height, n))
    return np.stack([x, y, z], 1).astype(np.float32)


@pytest.mark.parametrize("shape", ["line", "corridor", "ground"])
def test_degenerate_newton_system(oracle, shape):
    """Rank-deficient / ill-conditioned H: the reference solves H dp = -g with JacobiSVD, whose
    rank truncation only matters when cond_2(H) > 1/(6 eps); the device takes its LU solve only when kappa_1(H) proves
    that cannot happen and otherwise the Eigen-semantics SVD (solver_fallbacks counts those).  Per-pass parity with
    the oracle (which always uses JacobiSVD) on a line target (exactly degenerate: fallbacks must occur), a corridor
    and a flat ground-only target."""
    rng = np.random.default_rng(11)
    if shape == "line":
        tgt = _line_world(rng, 3000, -20, 20)
        src = _line_world(rng, 600, -10, 10)
        guess = np.eye(4)
        guess[0, 3] = 0.3
    elif shape == "corridor":
        tgt = _corridor(rng, 20000)
        src = _corridor(rng, 3000, half_len=10.0)
        guess = np.array(__import__("xchu_slam_amd").synth.pose_matrix(0.2, 0.1, 0.05, 0.0, 0.0, 0.02))
    else:
        xy = rng.uniform(-20, 20, (20000, 2))
        tgt = np.concatenate([xy, np.full((len(xy), 1), 0.37)], 1).astype(np.float32)   # a flat plane inside a cell row
        sxy = rng.uniform(-12, 12, (3000, 2))
        src = np.concatenate([sxy, np.full((len(sxy), 1), 0.37)], 1).astype(np.float32)
        guess = np.array(__import__("xchu_slam_amd").synth.pose_matrix(0.3, -0.2, 0.1, 0.01, -0.01, 0.03))
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=0.0, max_iter=10)
    o = oracle.OracleNDT(num_threads=1, **prm)
    o.set_target(tgt)
    o.set_source(src)
    g = xa.NormalDistributionsTransform()
    for k, v in prm.items():
        setattr(g._params, k, v)
    g._push()
    g.setInputTarget(tgt)
    g.setInputSource(src)
    ro = o.align(guess)
    g.align(guess, want_output=False)
    rg = g.result()
    ho, hg = o.history(), g.history()
    assert rg["nr_iterations"] == ro["nr_iterations"] and rg["converged"] == ro["converged"]
    assert len(ho) == len(hg)
    for a, b in zip(ho, hg):
        assert a["kind"] == b["kind"]
        assert np.max(np.abs(a["x"] - b["x"])) < X_TOL
    assert np.max(np.abs(rg["final_tf"] - ro["final_tf"])) < TF_TOL
    if shape == "line":
        assert rg["solver_fallbacks"] > 0


def test_radius_search_beyond_candidate_list(oracle):
    """KDTREE neighbours with radius = resolution on a grid built at a smaller leaf (setResolution before
    setInputSource keeps the old grid, ndt_omp.h:127-137): more centroids lie within the radius than the sorted list
    holds; they are visited exhaustively (never truncated) — same pair counts and per-pass parameters as the oracle,
    and calculateScore to 1e-12."""
    rng = np.random.default_rng(4)
    # a volume filled with points: every 1 m cell occupied, ~65 centroids within 2.5 m of an interior point
    tgt = rng.uniform([-6, -6, -3], [6, 6, 3], (50000, 3)).astype(np.float32)
    src = rng.uniform([-3, -3, -1.5], [3, 3, 1.5], (1500, 3)).astype(np.float32)
    from xchu_slam_amd import synth
    pair = synth.Pair(target=tgt, source=src, true_pose=np.eye(4), guess=synth.pose_matrix(0.1, -0.05, 0.02, 0.01, 0.0, 0.02))
    prm = dict(step_size=0.1, trans_eps=0.0, max_iter=3, search=xa.KDTREE)
    o = oracle.OracleNDT(num_threads=1, resolution=1.0, **prm)
    o.set_target(pair.target)
    o.set(resolution=2.5)          # no source yet: the grid keeps its 1.0 m leaf
    o.set_source(pair.source)
    g = xa.NormalDistributionsTransform()
    for k, v in prm.items():
        setattr(g._params, k, v)
    g._push()
    g.setInputTarget(pair.target)
    g.setResolution(2.5)
    g.setInputSource(pair.source)
    assert g.grid_info()["n_cloud"] == o.grid_header()["n_cloud"]
    # some points have more than 48 centroids within 2.5 m (the sorted list's capacity)
    leaves = o.grid_leaves()
    cen = leaves["centroid"][(leaves["npts"] >= 6) | (leaves["npts"] == -1)].astype(np.float64)
    xt = pair.source.astype(np.float64) @ pair.guess[:3, :3].T + pair.guess[:3, 3]
    d2 = ((xt[:200, None, :] - cen[None, :, :]) ** 2).sum(-1)
    assert (d2 < 2.5 * 2.5).sum(1).max() > 48
    ro = o.align(pair.guess)
    g.align(pair.guess, want_output=False)
    ho, hg = o.history(), g.history()
    assert g.result()["nr_iterations"] == ro["nr_iterations"] and len(ho) == len(hg)
    assert ho[0]["pairs"] == hg[0]["pairs"]
    for a, b in zip(ho, hg):
        assert np.max(np.abs(a["x"] - b["x"])) < X_TOL
    T = pair.guess.astype(np.float32)
    so, sg = o.calculate_score(T), g.calculateScore(T)
    assert abs(sg - so) <= 1e-12 * abs(so)


def _cpu_backend_pair(oracle, pair, **prm):
    o = oracle.OracleNDT(num_threads=1, precision_mode=2, **prm)
    g = xa.CpuNormalDistributionsTransform()
    for k, v in prm.items():
        setattr(g._params, k, v)
    g._push()
    return o, g


def _grid_parity_cpu(o, g):
    """cpu::VoxelGrid on the device vs the oracle: keys / counts / f64 centroids bit-exact, inverse covariances to
    1e-10 (the closed-form eigen solver's acos/cos run in the device math library)."""
    ol, gl = o.grid_leaves(), g.grid_leaves()
    sel = (ol["npts"] >= 6) | (ol["npts"] == -1)
    for k in ("keys", "npts", "mean"):
        assert np.array_equal(ol[k][sel], gl[k]), k
    valid = gl["npts"] > 0
    assert rel_err(gl["icov"][valid], ol["icov"][sel][valid]) < 1e-10


@pytest.mark.parametrize("eps", [0.0, 0.01])
def test_ndt_cpu_backend(oracle, eps):
    """ndt_cpu (cpu::NormalDistributionsTransform, odom_node's launch default ndt_method_type 1): the device grid as
    cpu::VoxelGrid builds it and every pass of the align (radius neighbours over f64 centroids, f64 pair math) vs the
    oracle's restatement — per-pass parameters to 1e-6, identical iterations and pair counts on the first pass."""
    pair = small_pair()
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=eps, max_iter=20)
    o, g = _cpu_backend_pair(oracle, pair, **prm)
    o.set_target(pair.target)
    o.set_source(pair.source)
    g.setInputTarget(pair.target)
    g.setInputSource(pair.source)
    _grid_parity_cpu(o, g)
    ro = o.align(pair.guess)
    g.align(pair.guess, want_output=False)
    rg, ho, hg = g.result(), o.history(), g.history()
    assert rg["nr_iterations"] == ro["nr_iterations"] and rg["converged"] == ro["converged"] and len(ho) == len(hg)
    assert ho[0]["pairs"] == hg[0]["pairs"] > 0
    for a, b in zip(ho, hg):
        assert a["kind"] == b["kind"]
        assert np.max(np.abs(a["x"] - b["x"])) < X_TOL
        assert a["pairs"] == b["pairs"]
    assert np.max(np.abs(rg["final_tf"] - ro["final_tf"])) < TF_TOL
    t_err, r_err = pose_err(rg["final_tf"], pair.true_pose)
    assert t_err < 0.2 and r_err < 0.5


def test_ndt_cpu_update_voxel_grid(oracle):
    """cpu::NormalDistributionsTransform::updateVoxelGrid (odom_node.cpp:344-345): the device appends the points and
    rebuilds; the oracle scatters them into its kept sums as ndt_cpu does — same grid and the same align; then a
    host-cloud update and a device-cloud update agree."""
    pair = small_pair(seed=7)
    half = len(pair.target) // 2
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=0.0, max_iter=8)
    o, g = _cpu_backend_pair(oracle, pair, **prm)
    o.set_target(pair.target[:half])
    o.update_target(pair.target[half:])
    o.set_source(pair.source)
    g.setInputTarget(pair.target[:half])
    g.updateVoxelGrid(pair.target[half:])
    g.setInputSource(pair.source)
    _grid_parity_cpu(o, g)
    ro = o.align(pair.guess)
    g.align(pair.guess, want_output=False)
    assert g.getFinalNumIteration() == ro["nr_iterations"]
    assert np.max(np.abs(g.getFinalTransformation() - ro["final_tf"])) < TF_TOL
    # the same update from a device-resident cloud, on a ctx whose target was a caller device buffer
    g2 = xa.CpuNormalDistributionsTransform()
    for k, v in prm.items():
        setattr(g2._params, k, v)
    g2._push()
    d0 = g2.device_upload(np.concatenate([pair.target[:half], np.ones((half, 1), np.float32)], 1))
    d1 = g2.device_upload(np.concatenate([pair.target[half:], np.ones((len(pair.target) - half, 1), np.float32)], 1))
    g2.setInputTargetDevice(d0, half)
    g2.updateVoxelGridDevice(d1, len(pair.target) - half)
    g2.setInputSource(pair.source)
    g2.align(pair.guess, want_output=False)
    assert np.array_equal(g2.getFinalTransformation(), g.getFinalTransformation())


def test_update_target_strided_records():
    """ndt_update_target over 32-byte records (x, y, z first, the rest poisoned) gives the grid of the 16-byte call."""
    import ctypes as C
    pair = small_pair(seed=7)
    first, more = pair.target[:1500], pair.target[1500:2400]
    assert len(more) == 900
    infos = []
    for width in (4, 8):
        rows = np.full((len(more), width), np.nan, np.float32)
        rows[:, :3] = more[:, :3]
        g = xa.NormalDistributionsTransform()
        try:
            g.setResolution(2.0)
            g.setInputTarget(first)
            st = g._lib.ndt_update_target(g._ctx, rows.ctypes.data_as(C.POINTER(C.c_float)), len(rows), width * 4)
            assert st == 0
            infos.append(g.grid_info())
        finally:
            g.close()
    assert infos[0]["n_cloud"] > 0 and infos[0]["n_valid"] > 0
    assert infos[1] == infos[0]


def test_ndt_cpu_degenerate_voxels_never_rejected(oracle):
    """The ndt_cpu incremental quirk (a rejected voxel's points_per_voxel continues from -1 in updateVoxelGrid, so it
    can stay hidden from radiusSearch) needs a rejected voxel, and cpu::VoxelGrid cannot produce one: its covariance
    sums start at Identity (libndt_cpu.so scatterPointsToVoxelGrid, read as text), so every voxel of n >= 2 points has
    covariance (n-1)/n (S + I/n) with S >= 0 — eigenvalues >= (n-1)/n^2 > 0 — and ndt_cpu keeps min_points_per_voxel
    at 6.  Checked on the worst geometries (6+ identical points, collinear, coplanar voxels) through a build and an
    update that adds points to those voxels: no voxel rejected on either side, same grid, same align.  The device's
    rebuild-on-update is then exactly ndt_cpu's continuation.  Parity unpinned (published Autoware algorithm)."""
    rng = np.random.default_rng(31)
    base = small_pair(seed=9)
    deg = []
    for k in range(40):
        c = np.array([2.0 + (k % 8), 3.0 + (k // 8), 1.0], np.float32) + 0.5
        kind = k % 3
        if kind == 0:
            pts = np.repeat(c[None], 7, 0)                                  # one point, seven times
        elif kind == 1:
            t = rng.uniform(-0.4, 0.4, (8, 1)).astype(np.float32)
            pts = c + t * np.array([[1.0, 0.3, 0.0]], np.float32)           # collinear
        else:
            uv = rng.uniform(-0.4, 0.4, (9, 2)).astype(np.float32)
            pts = c + np.stack([uv[:, 0], uv[:, 1], np.zeros(9, np.float32)], 1)  # coplanar
        deg.append(pts.astype(np.float32))
    first = np.concatenate([base.target[: len(base.target) // 2]] + deg).astype(np.float32)
    more = np.concatenate([base.target[len(base.target) // 2:]] + [d[:3] for d in deg]).astype(np.float32)
    prm = dict(resolution=1.0, step_size=0.1, trans_eps=0.0, max_iter=6)
    o, g = _cpu_backend_pair(oracle, base, **prm)
    o.set_target(first)
    g.setInputTarget(first)
    assert not np.any(o.grid_leaves()["npts"] == -1) and not np.any(g.grid_leaves()["npts"] == -1)
    _grid_parity_cpu(o, g)
    o.update_target(more)
    g.updateVoxelGrid(more)
    assert not np.any(o.grid_leaves()["npts"] == -1) and not np.any(g.grid_leaves()["npts"] == -1)
    _grid_parity_cpu(o, g)
    o.set_source(base.source)
    g.setInputSource(base.source)
    ro = o.align(base.guess)
    g.align(base.guess, want_output=False)
    assert g.getFinalNumIteration() == ro["nr_iterations"]
    assert np.max(np.abs(g.getFinalTransformation() - ro["final_tf"])) < TF_TOL
