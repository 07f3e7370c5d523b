"""The derivative pass of sources above 262 144 points, at the sizes where its launch geometry changes shape, against the
CPU oracle (computeDerivatives, ndt_omp_impl.hpp:175-251; computeHessian :550-607; computeTransformation :66-172).

Such a source is re-sorted into target-cell order for an align, runs last-workgroup tails only, switches k_pass_direct
between four geometries (one / two points per thread in a tile loop, the one-tile grid of points_per_thread = 3, and
k_pass_radius beside them) and, on more than 1024 workgroups, sums its partials through the two-level hand-off
(ndt_control.h pass_handoff).  One world: a 112 890-point target at resolution 1.0; the source sizes sit at the bucket
edges (csrc/ndt_geom.h geom_points) that give the geometry each case names.  Every case first asserts through
ndt_pass_geometry that it reached that geometry — the sizes hold for 256 CUs; elsewhere the assertion names what it
found — and then compares one pass at the guess with the oracle: pair count equal, score / g / H within 1e-9 relative
(tests/test_gpu_fullsize.py's bars).  Align cases add test_align_source_order's per-pass bars: the same records, kinds
and Newton iterations, pairs equal, x within X_TOL, the final transform within TF_TOL.

Each case prints its worst differences ("margin ..." lines, pytest -s); DESIGN.md's test section records them.
"""
import functools
import os

import numpy as np
import pytest

from helpers import TF_TOL, X_TOL, rel_err, small_pair

pytestmark = pytest.mark.gpu

xa = pytest.importorskip("xchu_slam_amd")

NT = max(1, min(16, os.cpu_count() or 1))  # oracle threads
M_TARGET = 112_890
DIRECT, LEAD, RADIUS = 0, 1, 2


@functools.lru_cache(maxsize=2)
def _world(n_source):
    pair = small_pair(seed=5, half=60.0, max_range=40.0, n_source=n_source)
    assert len(pair.target) == M_TARGET and len(pair.source) == n_source
    return pair


def _device(pair, ppt=None, **prm):
    g = xa.NormalDistributionsTransform()
    for k, v in dict(resolution=1.0, **prm).items():
        setattr(g._params, k, v)
    g._push()
    if ppt is not None:
        g.set_pass_options(points_per_thread=ppt)
    g.setInputTarget(pair.target)
    g.setInputSource(pair.source)
    return g


def _oracle(oracle, pair, threads=NT, **prm):
    o = oracle.OracleNDT(num_threads=threads, resolution=1.0, **prm)
    o.set_target(pair.target)
    o.set_source(pair.source)
    return o


# one oracle evaluation per (source size, search, backend, settings), shared by the cases on the same inputs
_pass_cache, _hess_cache, _align_cache = {}, {}, {}


def _oracle_pass(oracle, n, **prm):
    key = (n, tuple(sorted(prm.items())))
    if key not in _pass_cache:
        pair = _world(n)
        o = _oracle(oracle, pair, **prm)
        _pass_cache[key] = o.derivatives(oracle.initial_p(pair.guess), pair.guess.astype(np.float32), True)
        o.close()
    return _pass_cache[key]


def _oracle_hessian(oracle, n, **prm):
    key = (n, tuple(sorted(prm.items())))
    if key not in _hess_cache:
        pair = _world(n)
        o = _oracle(oracle, pair, **prm)
        _hess_cache[key] = o.hessian_radius(oracle.initial_p(pair.guess), pair.guess.astype(np.float32))
        o.close()
    return _hess_cache[key]


def _oracle_align(oracle, n, threads=NT, **prm):
    key = (n, threads, tuple(sorted(prm.items())))
    if key not in _align_cache:
        pair = _world(n)
        o = _oracle(oracle, pair, threads=threads, **prm)
        _align_cache[key] = (o.align(pair.guess), o.history())
        o.close()
    return _align_cache[key]


def _reached(g, which, **want):
    """The geometry the ctx launches for kernel `which` is the one the case is about."""
    got = g.pass_geometry(which)
    name = ("k_pass_direct", "k_pass_lead", "k_pass_radius")[which]
    assert {k: got[k] for k in want} == want, f"{name} launches {got}"
    return got


def _pass_parity(oracle, g, n, label, **prm):
    pair = _world(n)
    p = oracle.initial_p(pair.guess)
    T = pair.guess.astype(np.float32)
    so, go, Ho, Po = _oracle_pass(oracle, n, **prm)
    sg, gg, Hg, Pg = g.computeDerivatives(p, T, True)
    es, eg, eh = abs(so - sg) / abs(so), rel_err(gg, go), rel_err(Hg, Ho)
    print(f"margin {label}: pairs {Pg} (oracle {Po}) score {es:.2e} g {eg:.2e} H {eh:.2e}  bars 1e-9")
    assert Po == Pg and Po > n // 4
    assert es <= 1e-9 and eg < 1e-9 and eh < 1e-9
    return Pg


def _align_parity(oracle, g, n, label, threads=NT, **prm):
    pair = _world(n)
    ro, ho = _oracle_align(oracle, n, threads=threads, **prm)
    g.align(pair.guess, want_output=False)
    rg, hg = g.result(), g.history()
    assert rg["nr_iterations"] == ro["nr_iterations"] and len(hg) == len(ho)
    ex = max(float(np.max(np.abs(a["x"] - b["x"]))) for a, b in zip(ho, hg))
    etf = float(np.max(np.abs(rg["final_tf"] - ro["final_tf"])))
    print(f"margin {label}: {len(hg)} passes, x {ex:.2e} (bar {X_TOL:g}) final_tf {etf:.2e} (bar {TF_TOL:g})")
    for a, b in zip(ho, hg):
        assert a["kind"] == b["kind"] and a["newton_iter"] == b["newton_iter"]
        assert a["pairs"] == b["pairs"]
        assert np.max(np.abs(a["x"] - b["x"])) < X_TOL
    assert etf < TF_TOL
    return hg


# ---------------------------------------------------------------------------------------------- single passes
@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1"])
def test_one_tile_grid_one_level(oracle, search):
    """200 000 points, points_per_thread = 3: k_pass_direct<S, 1, true> on 784 one-tile workgroups, the only way to that
    instantiation; 784 <= 1024, so the partials are summed in one level."""
    n, s = 200_000, getattr(xa, search)
    g = _device(_world(n), ppt=3, search=s)
    _reached(g, DIRECT, workgroups=784, block=256, ppb=256, points_per_thread=1, one_tile=True, tiles=1, groups=0)
    _pass_parity(oracle, g, n, f"one-tile 784 {search}", search=s)
    g.close()


@pytest.mark.parametrize("n", [266_240, 262_145])
def test_one_tile_grid_two_level(oracle, n):
    """The top and the bottom of the first size bucket above 262 144 points: 1040 one-tile workgroups, 17 groups of the
    two-level hand-off, the last one of 16 workgroups; at 262 145 points that group holds one point (the bucket's other 4095 slots are empty)."""
    g = _device(_world(n), ppt=3, search=xa.DIRECT7)
    got = _reached(g, DIRECT, workgroups=1040, block=256, ppb=256, points_per_thread=1, one_tile=True, tiles=1, groups=17,
                   group_size=64)
    assert got["workgroups"] - 16 * got["group_size"] == 16
    _pass_parity(oracle, g, n, f"one-tile 1040 N={n}", search=xa.DIRECT7)
    g.close()


def test_radius_two_level_kdtree(oracle):
    """KDTREE at 266 240 points: k_pass_radius on 1040 workgroups takes the two-level hand-off by default, for the
    derivative pass and for computeHessian's radius pass."""
    n = 266_240
    pair = _world(n)
    g = _device(pair, search=xa.KDTREE)
    _reached(g, RADIUS, workgroups=1040, block=256, tiles=1, groups=17, group_size=64)
    _pass_parity(oracle, g, n, "radius 1040 KDTREE", search=xa.KDTREE)
    Ho, Po = _oracle_hessian(oracle, n, search=xa.KDTREE)
    Hg, Pg = g.computeHessianRadius(oracle.initial_p(pair.guess), pair.guess.astype(np.float32))
    eh = rel_err(Hg, Ho)
    print(f"margin radius 1040 computeHessian: pairs {Pg} (oracle {Po}) H {eh:.2e}  bar 1e-9")
    assert Po == Pg and Po > n // 4
    assert eh < 1e-9
    g.close()


def test_radius_two_level_pcl_ndt(oracle):
    """The pcl_ndt backend (precision_mode 1: f64 per pair, radius neighbours) at 266 240 points: the same 1040-workgroup
    two-level k_pass_radius."""
    n = 266_240
    g = _device(_world(n), precision_mode=1)
    _reached(g, RADIUS, workgroups=1040, block=256, tiles=1, groups=17, group_size=64)
    _pass_parity(oracle, g, n, "radius 1040 pcl_ndt", precision_mode=1)
    g.close()


def test_points_per_thread_on_one_source(oracle):
    """394 000 points through all three points_per_thread options on the same inputs: 1 = 512 workgroups walking four
    194-point tiles, 2 = 512 workgroups walking two 388-point tiles in 512 slots (the second slot of threads 132..255
    stays empty), 3 = 1552 one-tile workgroups in 25 groups.  Three summation orders, one pair set."""
    n = 394_000
    pair = _world(n)
    want = {1: dict(workgroups=512, block=256, ppb=194, points_per_thread=1, one_tile=False, tiles=4, groups=0),
            2: dict(workgroups=512, block=256, ppb=388, points_per_thread=2, one_tile=False, tiles=2, groups=0),
            3: dict(workgroups=1552, block=256, ppb=256, points_per_thread=1, one_tile=True, tiles=1, groups=25, group_size=64)}
    pairs = {}
    for ppt in (1, 2, 3):
        g = _device(pair, ppt=ppt, search=xa.DIRECT7)
        _reached(g, DIRECT, **want[ppt])
        pairs[ppt] = _pass_parity(oracle, g, n, f"394000 ppt={ppt}", search=xa.DIRECT7)
        g.close()
    assert pairs[1] == pairs[2] == pairs[3]


def test_two_points_per_thread_direct1(oracle):
    """k_pass_direct<S_DIRECT1, 2, false> (the default above 393 216 points) at 394 000 points."""
    n = 394_000
    g = _device(_world(n), ppt=2, search=xa.DIRECT1)
    _reached(g, DIRECT, workgroups=512, block=256, ppb=388, points_per_thread=2, one_tile=False, tiles=2, groups=0)
    _pass_parity(oracle, g, n, "394000 DIRECT1 ppt=2", search=xa.DIRECT1)
    g.close()


def test_radius_at_its_workgroup_cap(oracle):
    """KDTREE at 540 000 points: k_pass_radius at its 2048-workgroup cap (two grid-stride rounds), 32 full groups."""
    n = 540_000
    g = _device(_world(n), search=xa.KDTREE)
    _reached(g, RADIUS, workgroups=2048, block=256, tiles=2, groups=32, group_size=64)
    _pass_parity(oracle, g, n, "radius 2048 KDTREE", search=xa.KDTREE)
    g.close()


def test_one_tile_grid_above_4096_workgroups(oracle):
    """1 050 000 points, points_per_thread = 3: 4160 workgroups, the first grid whose group size ceil(nb / 64) = 65 was
    odd — group g's columns then started at an odd offset, which breaks the 16-byte alignment reduce_partials_block's
    paired loads need.  group_size rounds up to even: 64 groups of 66 (the last of 2)."""
    n = 1_050_000
    g = _device(_world(n), ppt=3, search=xa.DIRECT7)
    got = _reached(g, DIRECT, workgroups=4160, block=256, ppb=256, points_per_thread=1, one_tile=True, tiles=1, groups=64,
                   group_size=66)
    assert got["group_size"] % 2 == 0
    _pass_parity(oracle, g, n, "one-tile 4160", search=xa.DIRECT7)
    g.close()


# ---------------------------------------------------------------------------------------------- aligns
NEWTON = dict(step_size=0.1, trans_eps=0.0, max_iter=2)


def test_align_one_tile_grid_two_level(oracle):
    """A two-iteration align at 266 240 points with points_per_thread = 3: the source in target-cell order, every pass's
    Newton step (mode 0) run by the final closer of the two-level hand-off."""
    n = 266_240
    g = _device(_world(n), ppt=3, search=xa.DIRECT7, **NEWTON)
    _reached(g, DIRECT, workgroups=1040, one_tile=True, tiles=1, groups=17, group_size=64)
    _pass_parity(oracle, g, n, "align one-tile 1040: pass", search=xa.DIRECT7)
    _align_parity(oracle, g, n, "align one-tile 1040", search=xa.DIRECT7, **NEWTON)
    g.close()


def test_align_radius_two_level(oracle):
    """A two-iteration KDTREE align at 266 240 points: a chain of source-ordered two-level k_pass_radius passes."""
    n = 266_240
    g = _device(_world(n), search=xa.KDTREE, **NEWTON)
    _reached(g, RADIUS, workgroups=1040, tiles=1, groups=17, group_size=64)
    _pass_parity(oracle, g, n, "align radius 1040: pass", search=xa.KDTREE)
    _align_parity(oracle, g, n, "align radius 1040", search=xa.KDTREE, **NEWTON)
    g.close()


def test_align_more_thuente_direct_and_radius(oracle):
    """step_size 0.001 < trans_eps / 2: the More-Thuente loop runs, so one chain holds k_pass_direct (512 workgroups x
    three tiles) and the two-level k_pass_radius (computeHessian) — gradient-only and Hessian-only passes included.

    With step_min above step_max every trial of a line search evaluates the same point, and computeStepLengthMT's path
    then hangs on whether repeated evaluations give the same bits.  The device's do (fixed summation orders); the
    oracle's do only on one thread (its OpenMP loop is the reference's schedule(guided, 8): at 16 threads the second
    line search took 2 or 10 trials from run to run, 17 or 25 passes).  So this align's oracle runs on one thread, as
    in tests/test_gpu_parity.py, where the align bars come from."""
    n = 266_240
    prm = dict(step_size=0.001, trans_eps=2.0, max_iter=2)
    g = _device(_world(n), search=xa.DIRECT7, **prm)
    _reached(g, DIRECT, workgroups=512, ppb=174, points_per_thread=1, one_tile=False, tiles=3, groups=0)
    _reached(g, RADIUS, workgroups=1040, tiles=1, groups=17, group_size=64)
    _pass_parity(oracle, g, n, "align More-Thuente: pass", search=xa.DIRECT7)
    hg = _align_parity(oracle, g, n, "align More-Thuente", threads=1, search=xa.DIRECT7, **prm)
    kinds = {h["kind"] for h in hg}
    assert {1, 2} <= kinds, kinds
    g.close()


@pytest.mark.parametrize("ppt", [1, 2])
def test_align_tile_loops(oracle, ppt):
    """A two-iteration align at 394 000 points through the four-tile one-point-per-thread loop and through the
    two-points-per-thread kernel (both against one oracle align)."""
    n = 394_000
    g = _device(_world(n), ppt=ppt, search=xa.DIRECT7, **NEWTON)
    _reached(g, DIRECT, workgroups=512, ppb=194 * ppt, points_per_thread=ppt, one_tile=False, tiles=4 // ppt, groups=0)
    _pass_parity(oracle, g, n, f"align 394000 ppt={ppt}: pass", search=xa.DIRECT7)
    _align_parity(oracle, g, n, f"align 394000 ppt={ppt}", search=xa.DIRECT7, **NEWTON)
    g.close()
