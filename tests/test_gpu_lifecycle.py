"""Everything a registration context can own, alive at teardown: the side lanes, the ICP state, the profiling read-back
blocks, the batched replay's helper contexts and one handle of every kind, created and torn down three times in one
process.  Every number of a cycle is bitwise the first cycle's."""
import struct

import numpy as np
import pytest

from helpers import small_pair

pytestmark = pytest.mark.gpu


def frozen(x):
    """A value as nested tuples of bytes, so that == compares bit for bit (NaNs and signed zeros included)."""
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, float):
        return struct.pack("d", x)
    if isinstance(x, (np.ndarray, np.generic)):
        a = np.ascontiguousarray(x)
        return (a.dtype.str, a.shape, a.tobytes())
    return x


def one_cycle(xa, pair, first):
    from xchu_slam_amd import synth
    out = {}
    g = xa.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(30)
    g.setProfiling(True)

    def align():
        g.setInputTarget(pair.target)
        g.setInputSource(pair.source)
        g.align(pair.guess, want_output=False)
        return g.getFinalTransformation()

    out["align"] = align()
    out["history"] = g.history()
    out["fitness"] = g.getFitnessScore()                      # creates the side lanes
    icp = xa.IterativeClosestPoint(registration=g)
    icp.setMaximumIterations(5)
    icp.align(pair.guess, want_output=False)
    out["icp"] = (icp.getFinalTransformation(), icp.getFinalNumIteration(), icp.history())
    # four pairs through the batched replay (creates the helper contexts)
    d_t, d_s = g.device_upload(synth.to_xyz4(pair.target)), g.device_upload(synth.to_xyz4(pair.source))
    guesses = []
    for k in range(4):
        gk = np.array(pair.guess, np.float32)
        gk[0, 3] += np.float32(0.05 * k)
        guesses.append(gk)
    out["batch"] = g.align_batch([(d_t, len(pair.target), d_s, len(pair.source), gk) for gk in guesses])
    g.setInputTarget(pair.target)                             # the ctx lets go of the device clouds before they are freed
    g.setInputSource(pair.source)
    g.device_free(d_t)
    g.device_free(d_s)
    # one handle of every kind on the same context; 70 adds cross the databases' first growth step (64 slots)
    sc = xa.SCManager(registration=g)
    isc = xa.ISCGeneration(registration=g)
    pg = xa.PoseGraph(registration=g)
    for k in range(70):
        part = pair.source[40 * k: 40 * k + 40]
        sc.makeAndSaveScancontextAndKeys(part)
        isc.makeAndSavedec(np.column_stack([part, np.full(len(part), 0.1 * (k % 9), np.float32)]).astype(np.float32), (k, 0, 0))
    sc.detectLoopClosureID()
    isc.detectLoopClosureID()
    out["sc"], out["isc"] = sc.last_result(), isc.last_result()
    for k in range(5):
        pg.add_node((1.0 * k, 0.02 * k * k, 0.0, 0.0, 0.0, 0.01 * k))
    pg.add_loop(0, 4, (4.1, 0.2, 0.0, 0.0, 0.0, 0.05), 0.1)
    out["pgo"] = (pg.optimize(), pg.poses())
    if first:
        # a handle created on a context and closed alone leaves the context usable
        extra = xa.SCManager(registration=g)
        extra.makeAndSaveScancontextAndKeys(pair.source[:40])
        extra.close()
        assert frozen(align()) == frozen(out["align"])
    for obj in (sc, isc, pg, icp):
        obj.close()
    g.close()
    if first:
        for obj in (sc, isc, pg, icp, g):
            obj.close()                                       # a second close() is a no-op
    return frozen(out)


def test_everything_alive_at_teardown():
    import xchu_slam_amd as xa
    pair = small_pair(seed=3)
    first = one_cycle(xa, pair, True)
    for _ in range(2):
        again = one_cycle(xa, pair, False)
        for (k, a), (_, b) in zip(first, again):
            assert a == b, k
