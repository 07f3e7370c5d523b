"""Numpy restatement of Scan Context as pgo_node uses it (xchu_mapping/include/scancontext/Scancontext.{h,cpp} with
nanoflann's L2_Adaptor): the oracle of tests/test_gpu_scancontext.py.  Written from the semantics recorded in DESIGN.md
§2; the reference cannot be compiled here (no Eigen, no PCL), so parity with it is unpinned.

What is modelled, not restated: atanf = the f64 arctangent rounded to f32; every Eigen reduction (sum, dot, squaredNorm)
in Eigen 3.3's SSE2 order for sizes that are a multiple of four (four lane sums L_k = x_k + x_{k+4} + ..., then
(L0 + L2) + (L1 + L3)); equal ring-key distances go to the lower index.
"""
import math

import numpy as np

N_RING, N_SECTOR = 20, 60
MAX_RADIUS = 80.0
LIDAR_HEIGHT = 2.0
NO_POINT = -1000.0
BIG = 10000000.0            # the reference's "something large" initial minimum
K_DEG = 180 / math.pi       # (180/M_PI), a double
DEFAULTS = dict(dist_thres=0.2, num_exclude_recent=30, num_candidates=3, tree_making_period=30, search_ratio=0.1)

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ Eigen reductions
def esum(v):
    """Sum over the last axis (a multiple of four long) in Eigen 3.3's SSE2 linear-vectorised order."""
    v = np.asarray(v, f64)
    q = v.reshape(v.shape[:-1] + (v.shape[-1] // 4, 4))
    lane = q[..., 0, :].copy()
    for k in range(1, q.shape[-2]):
        lane = lane + q[..., k, :]
    return (lane[..., 0] + lane[..., 2]) + (lane[..., 1] + lane[..., 3])


def edot(a, b):
    return esum(np.asarray(a, f64) * np.asarray(b, f64))


def enorm(v):
    v = np.asarray(v, f64)
    return np.sqrt(esum(v * v))


# ------------------------------------------------------------------------------------------------ makeScancontext
def _bins(x, y, atan_ulps=0):
    """(ring, sector, kept, r) per point, 1-based as the reference computes them; atan_ulps moves the f64 arctangent by
    that many ulps before it is narrowed to f32 (the sensitivity report)."""
    x = np.asarray(x, f32)
    y = np.asarray(y, f32)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)                      # f32 throughout
        q1 = (x >= 0) & (y >= 0)
        q2 = (x < 0) & (y >= 0)
        q3 = (x < 0) & (y < 0)
        quot = np.where(q1 | q3, y / x, np.where(q2, y / (-x), (-y) / x)).astype(f32)
        at = np.arctan(quot.astype(f64))
        for _ in range(abs(atan_ulps)):
            at = np.nextafter(at, np.inf if atan_ulps > 0 else -np.inf)
        a = at.astype(f32).astype(f64)                  # atanf's result, widened for the double product
        ka = K_DEG * a
        theta = np.where(q1, ka, np.where(q2, 180.0 - ka, np.where(q3, 180.0 + ka, 360.0 - ka))).astype(f32)
        kept = ~(r > f32(MAX_RADIUS))
        ring = _ceil_clamp((r.astype(f64) / MAX_RADIUS) * N_RING, N_RING)
        sector = _ceil_clamp((theta.astype(f64) / 360.0) * N_SECTOR, N_SECTOR)
    return ring, sector, kept, r


def _ceil_clamp(v, hi):
    """max(min(hi, int(ceil(v))), 1); a NaN converts to INT_MIN on x86, which the clamp takes to 1."""
    c = np.ceil(v)
    c = np.where(np.isnan(c), -1.0, c)
    return np.clip(c, 1, hi).astype(np.int64)


def make_scancontext(points):
    """The 20 x 60 descriptor (f64 entries holding f32 values) of an (N, >=3) f32 cloud."""
    p = np.asarray(points, f32)
    if p.size == 0:
        p = np.zeros((0, 3), f32)
    desc = np.full((N_RING, N_SECTOR), NO_POINT, f64)
    if len(p):
        zp = (p[:, 2].astype(f64) + LIDAR_HEIGHT).astype(f32)
        ring, sector, kept, _ = _bins(p[:, 0], p[:, 1])
        flat = (ring[kept] - 1) * N_SECTOR + (sector[kept] - 1)
        np.maximum.at(desc.reshape(-1), flat, zp[kept].astype(f64))
    desc[desc == NO_POINT] = 0.0
    return desc


def bin_sensitive(points):
    """Indices of the points whose bin (or whose being kept at all) changes when the f64 arctangent moves by +-4 ulp
    before narrowing, or when r moves by one f32 ulp across a ring edge or 80.0: the inputs on which another libm could
    legitimately differ."""
    p = np.asarray(points, f32)
    if len(p) == 0:
        return np.zeros(0, np.int64)
    ring, sector, kept, r = _bins(p[:, 0], p[:, 1])
    bad = np.zeros(len(p), bool)
    for u in (-4, 4):
        _, s2, _, _ = _bins(p[:, 0], p[:, 1], atan_ulps=u)
        bad |= s2 != sector
    with np.errstate(all="ignore"):
        for r2 in (np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))):
            bad |= _ceil_clamp((r2.astype(f64) / MAX_RADIUS) * N_RING, N_RING) != ring
            bad |= (~(r2 > f32(MAX_RADIUS))) != kept
    return np.nonzero(bad)[0]


# ------------------------------------------------------------------------------------------------ keys
def ring_key(desc):
    """Row means, narrowed to f32 (eig2stdvec)."""
    return (esum(desc) / f64(N_SECTOR)).astype(f32)


def sector_key(desc):
    """Column means, f64."""
    return esum(desc.T) / f64(N_RING)


def column_norms(desc):
    return enorm(desc.T)


# ------------------------------------------------------------------------------------------------ distances
def circshift(m, s):
    """Columns moved right by s: out[:, (c + s) % n] = m[:, c]."""
    return np.roll(m, s, axis=-1)


def fast_align(vkey1, vkey2):
    """argmin over shifts 0..59 of |vkey1 - circshift(vkey2, s)|, first minimum."""
    norms = enorm(np.stack([vkey1 - circshift(vkey2, s) for s in range(N_SECTOR)]))
    best, arg = BIG, 0
    for s in range(N_SECTOR):
        if norms[s] < best:
            best, arg = float(norms[s]), s
    return arg


def dist_direct_shifts(sc1, sc2, shifts):
    """distDirectSC(sc1, circshift(sc2, s)) for every s of `shifts`: 1 - mean cosine similarity of the column pairs whose
    norms are both non-zero, the similarities added in column order (NaN when no pair counts)."""
    n1 = column_norms(sc1)
    sc2s = np.stack([circshift(sc2, s).T for s in shifts])          # (S, 60, 20)
    n2 = np.stack([circshift(column_norms(sc2), s) for s in shifts])
    dots = edot(sc1.T[None], sc2s)
    valid = (n1[None] != 0) & (n2 != 0)
    with np.errstate(all="ignore"):
        sim = dots / (n1[None] * n2)
        total = np.zeros(len(shifts), f64)
        for j in range(N_SECTOR):
            total = np.where(valid[:, j], total + sim[:, j], total)
        return f64(1.0) - total / valid.sum(1).astype(f64)


def dist_direct(sc1, sc2):
    return float(dist_direct_shifts(sc1, sc2, [0])[0])


def search_radius(search_ratio):
    """round(0.5 * SEARCH_RATIO * cols), C's round (half away from zero)."""
    return int(math.floor(0.5 * search_ratio * N_SECTOR + 0.5))


def distance(sc1, sc2, search_ratio=0.1):
    """distanceBtnScanContext -> (dist, shift)."""
    a = fast_align(sector_key(sc1), sector_key(sc2))
    rad = search_radius(search_ratio)
    space = [a]
    for i in range(1, rad + 1):
        space += [(a + i + N_SECTOR) % N_SECTOR, (a - i + N_SECTOR) % N_SECTOR]
    space = sorted(space)
    best, arg = BIG, 0
    for s, d in zip(space, dist_direct_shifts(sc1, sc2, space)):
        if d < best:
            best, arg = float(d), s
    return best, arg


def deg2rad_f32(deg):
    return f32(f64(f32(deg)) * math.pi / 180.0)


# ------------------------------------------------------------------------------------------------ detection
def ring_dist2(query, keys):
    """nanoflann L2_Adaptor in f32: per group of four, result += d0*d0 + d1*d1 + d2*d2 + d3*d3."""
    keys = np.asarray(keys, f32).reshape(-1, N_RING)
    d = (np.asarray(query, f32)[None, :] - keys).astype(f32)
    sq = d * d
    res = np.zeros(len(keys), f32)
    for g in range(0, N_RING, 4):
        res = res + (((sq[:, g] + sq[:, g + 1]) + sq[:, g + 2]) + sq[:, g + 3])
    return res


def empty_record():
    return dict(loop_id=-1, yaw_diff=f32(0.0), min_dist=BIG, nn_idx=0, nn_align=0, cand_idx=[], cand_dist=[], cand_shift=[],
                tie=False)


def detect_one(descs, rkeys, q, n_search, dist_thres=0.2, num_candidates=3, search_ratio=0.1, cache=None, **_):
    """One query against ring keys [0, n_search): the record detectLoopClosureID computes after its early return.
    cache: a dict that keeps distance(descs[q], descs[i]) per (q, i, search_ratio) between calls over the same descs."""
    if n_search <= 0:
        return empty_record()
    d2 = ring_dist2(rkeys[q], np.asarray(rkeys[:n_search]))
    order = np.lexsort((np.arange(n_search), d2))     # ascending distance, the lower index first among equals
    order = order[~np.isnan(d2[order])]
    cand = [int(i) for i in order[:num_candidates]]
    tie = len(order) > len(cand) and len(cand) > 0 and d2[order[len(cand)]] == d2[cand[-1]]
    rec = empty_record()
    for i in cand:
        key = (q, i, search_ratio)
        if cache is None or key not in cache:
            d, s = distance(descs[q], descs[i], search_ratio)
            if cache is not None:
                cache[key] = (d, s)
        else:
            d, s = cache[key]
        rec["cand_idx"].append(i)
        rec["cand_dist"].append(d)
        rec["cand_shift"].append(s)
        if d < rec["min_dist"]:
            rec.update(min_dist=d, nn_align=s, nn_idx=i)
    tie = bool(tie or len(set(rec["cand_dist"])) != len(rec["cand_dist"]))
    if rec["min_dist"] < dist_thres:
        rec["loop_id"] = rec["nn_idx"]
    rec["yaw_diff"] = deg2rad_f32(rec["nn_align"] * 6.0)
    rec["tie"] = tie
    return rec


def search_schedule(n, tree_making_period=30, num_exclude_recent=30):
    """n_search per keyframe for one detection after every add: the searchable set is rebuilt (to size - exclude) when
    the period counter is a multiple of the period; the early return does not advance the counter."""
    out, counter, searchable = [], 0, 0
    for q in range(n):
        size = q + 1
        if size < num_exclude_recent + 1:
            out.append(0)
            continue
        if counter % tree_making_period == 0:
            searchable = size - num_exclude_recent
        counter += 1
        out.append(searchable)
    return out


class SCManager:
    """The reference's object, restated: same method names, records kept for comparison."""

    def __init__(self, **params):
        self.prm = dict(DEFAULTS)
        self.prm.update(params)
        self.descs, self.rkeys, self.skeys = [], [], []
        self.counter = 0
        self.searchable = 0
        self.last = empty_record()

    def setSCdistThres(self, t):
        self.prm["dist_thres"] = float(t)

    def saveScancontextAndKeys(self, desc):
        desc = np.asarray(desc, f64).reshape(N_RING, N_SECTOR)
        self.descs.append(desc)
        self.rkeys.append(ring_key(desc))
        self.skeys.append(sector_key(desc))

    def makeAndSaveScancontextAndKeys(self, cloud):
        self.saveScancontextAndKeys(make_scancontext(cloud))

    def distanceBtnScanContext(self, i, j):
        return distance(self.descs[i], self.descs[j], self.prm["search_ratio"])

    def detectLoopClosureID(self):
        size = len(self.descs)
        if size < self.prm["num_exclude_recent"] + 1:
            self.last = empty_record()
            return -1, f32(0.0)
        if self.counter % self.prm["tree_making_period"] == 0:
            self.searchable = size - self.prm["num_exclude_recent"]
        self.counter += 1
        self.last = detect_one(self.descs, self.rkeys, size - 1, self.searchable, **self.prm)
        return self.last["loop_id"], self.last["yaw_diff"]


def detect_loops(descs, tree_making_period=1, cache=None, **params):
    """Batch form: every descriptor stored first, then one record per keyframe under the rebuild schedule."""
    prm = dict(DEFAULTS)
    prm.update(params)
    prm["tree_making_period"] = tree_making_period
    descs = [np.asarray(d, f64).reshape(N_RING, N_SECTOR) for d in descs]
    rkeys = [ring_key(d) for d in descs]
    sched = search_schedule(len(descs), tree_making_period, prm["num_exclude_recent"])
    return [detect_one(descs, rkeys, q, sched[q], cache=cache, **prm) for q in range(len(descs))]
