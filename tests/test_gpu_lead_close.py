"""How a leading-tail chain round ends (the round's extra k_pass_lead slot, which runs the step of the round's last pass,
and the k_readback launch behind it) against the last-workgroup tails (k_pass_direct, set_pass_options(lead_tail=0)):
transform, iteration and pass counts and every pass record bit for bit — both chains run the same arithmetic in the same
order, only where it runs differs.  Both kernels end their bodies in block_reduce_store_split (the 22-value
reduce-scatter, csrc/ndt_rstree.h) with different wave counts, so the records also compare its results across them.

Written for a one-workgroup closing kernel in place of that slot and of k_readback (measured and not kept,
profiles/lead_close/AB.md); the cases are those of a round's end either way: the source sizes at which the partial
columns summed at the end change shape (1 point; 63, 64, 65; exactly one and two workgroups with points; a last
workgroup with a single point), max_iter 1 and 2 (the round's end consumes the first passes of an align), rounds that
end with a pass still pending (continuation rounds, odd and even first-round lengths: both ping-pong parities),
profiling on and off, a DIRECT26 chain, the mirrored primary state (get_output, getFitnessScore), two contexts in
flight, and a flagged target build."""
import ctypes as C

import numpy as np
import pytest

from helpers import small_pair

pytestmark = pytest.mark.gpu

xa = pytest.importorskip("xchu_slam_amd")
from xchu_slam_amd._lib import NdtResult, check  # noqa: E402


@pytest.fixture(scope="module")
def pair():
    return small_pair(seed=5)


def _ctx(pair, lead_tail, iters=6, eps=0.0, search=None, source=None, profiling=False, **build):
    g = xa.NormalDistributionsTransform()
    g.set_pass_options(lead_tail=lead_tail)
    g.setResolution(1.0)
    g.setTransformationEpsilon(eps)
    g.setMaximumIterations(iters)
    g.setNeighborhoodSearchMethod(xa.DIRECT7 if search is None else search)
    if build:
        g.set_build_options(**build)
    if profiling:
        g.setProfiling(True)
    g.setInputTarget(pair.target)
    g.setInputSource(pair.source if source is None else source)
    return g


def _record(g):
    r = g.result()
    return {"tf": r["final_tf"].tobytes(), "iters": r["nr_iterations"], "passes": r["n_passes"], "pairs": r["n_pairs"],
            "score": r["score"], "converged": r["converged"],
            "hist": [(h["kind"], h["newton_iter"], h["score"], h["pairs"], h["x"].tobytes(), h["g"].tobytes(), h["H"].tobytes())
                     for h in g.history()]}


def _same(a, b, what=""):
    for k in ("iters", "passes", "pairs", "converged"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["tf"] == b["tf"], what
    assert np.float64(a["score"]).tobytes() == np.float64(b["score"]).tobytes(), what
    assert len(a["hist"]) == len(b["hist"]) == a["passes"] > 0, what
    for i, (ra, rb) in enumerate(zip(a["hist"], b["hist"])):
        assert ra == rb, (what, "pass", i)


def _sizes(pair):
    """Source sizes from the lead kernel's geometry: workgroups take ppb points each."""
    g = _ctx(pair, True, source=pair.source[:1])
    small = g.pass_geometry(1)
    g.setInputSource(pair.source[:2561])
    big = g.pass_geometry(1)
    g.close()
    ppb = small["ppb"]
    assert ppb == 64 and small["workgroups"] >= 2 and big["ppb"] == 64 and big["workgroups"] > 41, (small, big)
    # one workgroup with points (ppb), its neighbours, two (2 ppb); 40 full workgroups and a 41st with one point
    return [1, ppb - 1, ppb, ppb + 1, 2 * ppb, 40 * big["ppb"] + 1]


def test_sizes_from_geometry(pair):
    assert _sizes(pair) == [1, 63, 64, 65, 128, 2561]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 2561])
def test_source_sizes(pair, n):
    out = []
    for lead in (True, False):
        g = _ctx(pair, lead, source=pair.source[:n])
        g.align(pair.guess, want_output=False)
        first = _record(g)
        g.align(pair.guess, want_output=False)  # the chain's length now follows the first align's passes
        out.append((first, _record(g)))
        g.close()
    _same(out[0][0], out[1][0], f"n={n} first")
    _same(out[0][1], out[1][1], f"n={n} second")
    _same(out[0][0], out[0][1], f"n={n} first against second")


@pytest.mark.parametrize("iters", [1, 2])
def test_round_end_consumes_the_first_passes(pair, iters):
    out = []
    for lead in (True, False):
        g = _ctx(pair, lead, iters=iters)
        recs = []
        for _ in range(2):
            g.align(pair.guess, want_output=False)
            recs.append(_record(g))
        g.close()
        out.append(recs)
    for k in range(2):
        _same(out[0][k], out[1][k], f"max_iter={iters} align {k}")
    _same(out[0][0], out[0][1], f"max_iter={iters} first against second")


def _easy_then_hard(pair, lead, easy_iters, profiling=False):
    """An easy align (guess = true pose) of easy_iters iterations, then a hard one (30): the hard align's first round is
    easy passes + 2 kernels long, too short, so that it ends with a pass pending and continuation rounds follow.  Returns the record, the first round's length, the output cloud, the fitness score and the timings."""
    g = _ctx(pair, lead, iters=easy_iters, eps=0.0, profiling=profiling)
    g.align(pair.true_pose, want_output=False)
    easy_passes = g.result()["n_passes"]
    g.setMaximumIterations(30)
    if profiling:
        g.setProfiling(True)  # the statistics of the hard align alone
    cloud = g.align(pair.guess)
    rec, fit, tm = _record(g), g.getFitnessScore(), g.timings()
    g.close()
    return rec, max(3, easy_passes + 2), cloud, fit, tm


def test_continuation_rounds_both_parities(pair):
    lengths = set()
    for easy_iters in range(1, 7):  # no convergence test (eps 0): the easy align's passes grow with its iterations
        a, slots, cloud_a, fit_a, _ = _easy_then_hard(pair, True, easy_iters)
        b, _, cloud_b, fit_b, _ = _easy_then_hard(pair, False, easy_iters)
        _same(a, b, f"easy_iters={easy_iters}")
        assert a["passes"] > slots - 1, (a["passes"], slots)  # the first round ended with a pass pending
        # the transformed source and the fitness score read the primary state buffer the read-back mirrors into
        assert np.array_equal(cloud_a, cloud_b) and np.float64(fit_a).tobytes() == np.float64(fit_b).tobytes()
        lengths.add(slots & 1)
    assert lengths == {0, 1}, lengths


def test_profiling_on_and_off(pair):
    n = len(pair.source)
    plain, _, _, _, tm_off = _easy_then_hard(pair, True, 1)
    assert tm_off["ms_pass_avg"] == 0.0 and tm_off["pass_bytes_avg"] == 0.0 and not any(tm_off["pass_phases_ms"].values())
    prof, slots, _, _, tm = _easy_then_hard(pair, True, 1, profiling=True)
    _same(prof, plain, "profiling on against off")
    assert prof["passes"] > slots - 1  # rows read back by a continuation round too
    assert tm["ms_pass_avg"] > 0.0 and tm["ms_align"] > 0.0
    # every pass is timed (its end stamp is the next kernel's start, the last one's the round's extra kernel's): the mean of
    # 16 N + 36 pairs over the timed passes equals the mean over all pass records (integers: exact in f64)
    want = sum(16.0 * n + 36.0 * h[3] for h in prof["hist"]) / prof["passes"]
    assert tm["pass_bytes_avg"] == want, (tm["pass_bytes_avg"], want)
    # a chain that fits its first round
    g = _ctx(pair, True, iters=6, profiling=True)
    g.align(pair.guess, want_output=False)
    g.setProfiling(True)
    g.align(pair.guess, want_output=False)
    rec, tm = _record(g), g.timings()
    assert tm["pass_bytes_avg"] == sum(16.0 * n + 36.0 * h[3] for h in rec["hist"]) / rec["passes"] and tm["ms_pass_avg"] > 0.0
    # profiling off again on the same ctx: the chain gets no stamp buffer, and nothing is collected
    g.setProfiling(False)
    g.align(pair.guess, want_output=False)
    off = g.timings()
    _same(_record(g), rec, "profiling off after on")
    assert off["ms_pass_avg"] == 0.0 and off["pass_bytes_avg"] == 0.0
    g.close()


def test_direct26_chain(pair):
    out = []
    for lead in (True, False):
        g = _ctx(pair, lead, search=xa.DIRECT26)
        if lead:
            assert g.pass_geometry(1)["block"] == 256 and not g.pass_geometry(1)["one_tile"]
        g.align(pair.guess, want_output=False)
        out.append(_record(g))
        g.close()
    _same(out[0], out[1], "direct26")


def test_two_contexts_in_flight(pair):
    other = small_pair(seed=9)
    want = []
    for p in (pair, other):
        g = _ctx(p, False)
        g.align(p.guess, want_output=False)
        want.append(_record(g))
        g.close()
    ctxs = [_ctx(pair, True), _ctx(other, True)]
    guesses = [np.ascontiguousarray(np.asarray(p.guess, np.float32).T).reshape(-1) for p in (pair, other)]
    for rep in range(2):
        for g, q in zip(ctxs, guesses):
            check(g._lib.ndt_align_async(g.ctx, q.ctypes.data_as(C.POINTER(C.c_float))), g.ctx)
        for g in reversed(ctxs):
            res = NdtResult()
            check(g._lib.ndt_align_wait(g.ctx, C.byref(res)), g.ctx)
            g._result = res
        for g, w in zip(ctxs, want):
            _same(_record(g), w, f"async rep {rep}")
    for g in ctxs:
        g.close()


def test_flagged_build_is_reported_and_rerun():
    """Too few radix passes (forced, as tests/test_gpu_build_robustness.py does): the round's read-back carries the
    header's error bits, the build and the align are re-run, and the result is an unforced context's."""
    p = small_pair(seed=5, half=60.0, n_source=6000)
    ref = _ctx(p, True, iters=8)
    ref.align(p.guess, want_output=False)
    f = _ctx(p, True, iters=8, radix_passes=1)
    assert f.build_stats()["radix_passes"] == 1
    f.align(p.guess, want_output=False)
    st = f.build_stats()
    assert st["rerun"] == 1 and st["rerun_lookback"] == 0, st
    _same(_record(f), _record(ref), "flagged build")
    assert ref.build_stats()["rerun"] == 0
    ref.close()
    f.close()


@pytest.mark.parametrize("lead", [False, True])
def test_pass_phases_by_chain_kind(pair, lead):
    """What ndt_pass_phases reports of the product library, through the public API: a last-workgroup-tail chain stamps all
    eight slots of a pass row, so all seven phases are > 0; a leading-tail chain's kernel stamps a pass's start and end only
    (k_pass_lead hands tail_control no stamp pointer), so the passes are timed and every phase is 0.  Profiling changes
    nothing of the result."""
    g = _ctx(pair, lead)
    g.align(pair.guess, want_output=False)
    plain = _record(g)
    g.close()
    g = _ctx(pair, lead, profiling=True)
    g.align(pair.guess, want_output=False)
    rec, tm = _record(g), g.timings()
    g.close()
    _same(rec, plain, f"lead={lead} profiling on against off")
    assert tm["ms_pass_avg"] > 0.0, tm
    phases = tm["pass_phases_ms"]
    assert len(phases) == 7
    if lead:
        assert all(v == 0.0 for v in phases.values()), phases
    else:
        assert all(v > 0.0 for v in phases.values()), phases
