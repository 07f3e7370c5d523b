"""numpy restatement of filter_node's ground detection as the device implements it (DESIGN.md §2 "Ground":
CloudFilter::DetectPlane with PlaneClip and NormalFiltering, xchu_mapping/src/filter_node.cpp:53-216, over PCL 1.7's
PlaneClipper3D, NormalEstimation, RandomSampleConsensus and SampleConsensusModelPlane).  PCL is not available: this
restatement is the specification's executable form (parity with PCL unpinned).

What is modelled rather than known:
  * rnd() of the model's boost::uniform_int<>(0, INT_MAX) over boost::mt19937: the raw 32-bit word shifted right by one;
  * PCL's one-pass f32 covariance and pcl::eigen33: here f64 sums in neighbour order (f32 products), the smallest
    eigenvalue's vector of the f64 matrix (numpy's eigh; the device runs sym_eigen3);
  * tilt_matrix.inverse(): the rotation transposed;
  * the order of every f32 dot product: ((a x + b y) + c z) + d, no fused multiply-add; pow(w, 3) as (w w) w.
"""
import math

import numpy as np

from gicp_restate import cosf_dr, knn_bruteforce, knn_order, sinf_dr
from icp_restate import F32, transform_f32

DEFAULTS = dict(tilt_deg=0.0, sensor_height=2.0, height_clip_range=2.5, floor_pts_thresh=512, floor_normal_thresh=10.0,
                use_normal_filtering=True, normal_filter_thresh=20.0, normal_k=10, ransac_threshold=0.1, ransac_probability=0.99,
                ransac_max_iterations=1000, literal_no_ground=False)
REASONS = ("OK", "TOO_FEW_POINTS", "TOO_FEW_INLIERS", "NOT_VERTICAL")
SEED = 12345                 # SampleConsensusModel's generator, seeded anew for every scan's model
MAX_SAMPLE_CHECKS = 1000     # SampleConsensusModel::max_sample_checks_
DBL_EPS = float(np.finfo(np.float64).eps)
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ generator
class MT19937:
    """boost::mt19937: words() hands out the raw 32-bit outputs in order."""

    def __init__(self, seed=5489):
        mt = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xFFFFFFFF)
        self.mt, self.at = mt, 624

    def next(self) -> int:
        mt = self.mt
        if self.at == 624:
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.at = 0
        y = mt[self.at]
        self.at += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y

    def words(self, n) -> np.ndarray:
        return np.array([self.next() for _ in range(n)], np.uint32)


def rnd(gen: MT19937) -> int:
    """variate_generator<mt19937&, uniform_int<>(0, INT_MAX)>: a model, the raw word shifted right by one."""
    return gen.next() >> 1


# ------------------------------------------------------------------------------------------------ a. tilt, b. clip
def tilt_matrix(tilt_deg):
    """AngleAxisf(tilt_deg pi / 180, UnitY).toRotationMatrix() in a Matrix4f (the operations of ndt_linalg.h's
    angle_axis_sc), and its inverse as the transposed rotation."""
    angle = F32(tilt_deg * math.pi / 180.0)
    s, c = sinf_dr(angle), cosf_dr(angle)
    ax = np.array([0, 1, 0], F32)
    sa = (s * ax).astype(F32)
    c1 = (F32(F32(1) - c) * ax).astype(F32)
    R = np.zeros((3, 3), F32)
    t = c1[0] * ax[1]; R[0, 1] = t - sa[2]; R[1, 0] = t + sa[2]
    t = c1[0] * ax[2]; R[0, 2] = t + sa[1]; R[2, 0] = t - sa[1]
    t = c1[1] * ax[2]; R[1, 2] = t - sa[0]; R[2, 1] = t + sa[0]
    R[0, 0] = c1[0] * ax[0] + c; R[1, 1] = c1[1] * ax[1] + c; R[2, 2] = c1[2] * ax[2] + c
    T, Ti = np.eye(4, dtype=F32), np.eye(4, dtype=F32)
    T[:3, :3] = R
    Ti[:3, :3] = R.T
    return T, Ti


def move(T, cloud):
    """pcl::transformPointCloud of an (N, 4) cloud: x, y, z by the project's f32 expression, intensity carried."""
    cloud = np.asarray(cloud, F32)
    out = cloud.copy()
    if len(cloud):
        out[:, :3] = transform_f32(T, cloud[:, :3])
    return out


def clip_mask(cloud, sensor_height=2.0, height_clip_range=2.5):
    """The two PlaneClipper3D calls with planes (0, 0, 1, sensor_height +- range): kept by the first, not by the second;
    a clipper keeps plane . (x, y, z, 1) >= 0, the f32 dot product as written."""
    p = np.asarray(cloud, F32)
    z0, o1 = F32(0), F32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (z0 * p[:, 0] + z0 * p[:, 1]) + o1 * p[:, 2]
        a = dot + F32(sensor_height + height_clip_range)
        b = dot + F32(sensor_height - height_clip_range)
        return (a >= 0) & ~(b >= 0)


# ------------------------------------------------------------------------------------------------ c. normal filter
def normals(pts, k=10, vp_z=2.0, nn=None, reverse=False, exact=False):
    """pcl::NormalEstimation with setKSearch(k) and the viewpoint (0, 0, vp_z) over the cloud itself.  Returns a dict:
    nn (n, k') neighbour indices ascending (d2, index), normal (n, 3) f32 oriented to the viewpoint, absz (n,) f32 =
    |normalized(normal) . UnitZ|, ev (n, 3) ascending eigenvalues.  reverse: the sums run in the reversed neighbour
    order (the restatement's own spread).  Fewer than 3 neighbours: NaN."""
    pts = np.ascontiguousarray(np.asarray(pts, F32)[:, :3])
    n = len(pts)
    kk = min(k, n)
    out = dict(nn=np.zeros((n, kk), np.int64), normal=np.full((n, 3), np.nan, F32), absz=np.full(n, np.nan, F32),
               ev=np.full((n, 3), np.nan))
    if n == 0:
        return out
    if nn is None:
        nn = knn_bruteforce(pts, kk)[0] if exact else knn_order(pts, kk)[0]
    out["nn"] = nn
    if kk < 3:
        return out
    mean = np.zeros((n, 3))
    cov = np.zeros((n, 3, 3))
    order = range(kk - 1, -1, -1) if reverse else range(kk)
    for j in order:  # the sums run in neighbour order; each product is an f32 product added to an f64 sum
        p = pts[nn[:, j]]
        mean += p.astype(np.float64)
        for a in range(3):
            for b in range(a + 1):
                cov[:, a, b] += (p[:, a] * p[:, b]).astype(np.float64)
    mean /= float(kk)
    for a in range(3):
        for b in range(a + 1):
            cov[:, a, b] /= float(kk)
            cov[:, a, b] -= mean[:, a] * mean[:, b]
            cov[:, b, a] = cov[:, a, b]
    ev, V = np.linalg.eigh(cov)
    nrm = V[:, :, 0].astype(F32)
    # flipNormalTowardsViewpoint: flip when n . (vp - p) < 0, in f32
    v = np.stack([F32(0) - pts[:, 0], F32(0) - pts[:, 1], F32(vp_z) - pts[:, 2]], 1).astype(F32)
    cos_theta = (v[:, 0] * nrm[:, 0] + v[:, 1] * nrm[:, 1]) + v[:, 2] * nrm[:, 2]
    nrm[cos_theta < 0] *= F32(-1)
    # getNormalVector3fMap().normalized().dot(UnitZ) in f32
    length = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]).astype(F32)
    hat = (nrm / length[:, None]).astype(F32)
    dot = (hat[:, 0] * F32(0) + hat[:, 1] * F32(0)) + hat[:, 2] * F32(1)
    out.update(normal=nrm, absz=np.abs(dot).astype(F32), ev=ev)
    return out


def normal_keep(absz, normal_filter_thresh=20.0):
    """std::abs(dot) > std::cos(thresh pi / 180): the f32 value against the double."""
    with np.errstate(invalid="ignore"):
        return np.asarray(absz, F32).astype(np.float64) > math.cos(normal_filter_thresh * math.pi / 180.0)


def keep_margin(clipped, k=10, vp_z=2.0, normal_filter_thresh=20.0, exact=False):
    """Where the device's keep flag is held to the restatement's: everywhere but within a margin of the threshold.
    The margin is measured, ten times the restatement's own spread: the largest difference in |n.z| between the sums
    run forwards and backwards over the neighbours.  A point whose two smallest eigenvalues lie within the same
    relative spread ((ev1 - ev0) / ev2 <= margin) is excluded too: its normal is not determined.  Returns a dict:
    fwd (the forward `normals`), keep, margin, excluded (bool per point)."""
    fwd = normals(clipped, k, vp_z, exact=exact)
    rev = normals(clipped, k, vp_z, nn=fwd["nn"], reverse=True)
    with np.errstate(invalid="ignore"):
        margin = 10.0 * float(np.nanmax(np.abs(fwd["absz"].astype(np.float64) - rev["absz"].astype(np.float64))))
        cos_thr = math.cos(normal_filter_thresh * math.pi / 180.0)
        near = np.abs(fwd["absz"].astype(np.float64) - cos_thr) <= margin
        ev = fwd["ev"]
        degenerate = (ev[:, 1] - ev[:, 0]) <= margin * np.abs(ev[:, 2])
    return dict(fwd=fwd, keep=normal_keep(fwd["absz"], normal_filter_thresh), margin=margin, excluded=near | degenerate)


# ------------------------------------------------------------------------------------------------ e. RANSAC
def collinear(p0, p1, p2):
    """isSampleGood / computeModelCoefficients: the component-wise f32 ratios of p1 - p0 and p2 - p0 all equal."""
    with np.errstate(all="ignore"):
        r = ((np.asarray(p1, F32)[:3] - np.asarray(p0, F32)[:3]) / (np.asarray(p2, F32)[:3] - np.asarray(p0, F32)[:3])).astype(F32)
    return bool(r[0] == r[1] and r[2] == r[1])


def plane_of(p0, p1, p2):
    """computeModelCoefficients: the f32 cross product of the two differences, normalised, d = -(n . p0)."""
    p0, p1, p2 = (np.asarray(q, F32)[:3] for q in (p0, p1, p2))
    a, b = (p1 - p0).astype(F32), (p2 - p0).astype(F32)
    with np.errstate(all="ignore"):
        m = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)
        nrm = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]).astype(F32)
        m = (m / nrm).astype(F32)
        d = -((m[0] * p0[0] + m[1] * p0[1]) + m[2] * p0[2])
    return np.array([m[0], m[1], m[2], d], F32)


def plane_distance(coef, pts):
    """The f32 distance ((a x + b y) + c z) + d of every point."""
    c = np.asarray(coef, F32)
    p = np.asarray(pts, F32)
    with np.errstate(all="ignore"):
        return ((c[0] * p[:, 0] + c[1] * p[:, 1]) + c[2] * p[:, 2]) + c[3]


def within(coef, pts, thr=0.1):
    """countWithinDistance / selectWithinDistance: fabs(distance) < threshold, the float against the double."""
    with np.errstate(invalid="ignore"):
        return np.abs(plane_distance(coef, pts)).astype(np.float64) < thr


class Sampler:
    """SampleConsensusModel::getSamples for a model over n points: drawIndexSample's partial Fisher-Yates over the
    persistent shuffled_indices_ (kept sparsely: only touched positions), redrawn while isSampleGood fails."""

    def __init__(self, pts, seed=SEED):
        self.pts = np.asarray(pts, F32)
        self.n = len(self.pts)
        self.gen = MT19937(seed)
        self.shuffled = {}
        self.draws = 0

    def _get(self, j):
        return self.shuffled.get(j, j)

    def draw(self):
        for i in range(3):
            j = i + rnd(self.gen) % (self.n - i)
            self.draws += 1
            a, b = self._get(i), self._get(j)
            self.shuffled[i], self.shuffled[j] = b, a
        return tuple(self._get(i) for i in range(3))

    def sample(self):
        """A good sample, or None after MAX_SAMPLE_CHECKS draws ("No samples could be selected")."""
        for _ in range(MAX_SAMPLE_CHECKS):
            t = self.draw()
            if not collinear(self.pts[t[0]], self.pts[t[1]], self.pts[t[2]]):
                return t
        return None


def bound_k(count, n, log_probability):
    """k = log(1 - p) / log(clamp(1 - w^3)) with w = count / n."""
    w = float(count) * (1.0 / float(n))
    p_no_outliers = 1.0 - (w * w) * w
    p_no_outliers = max(DBL_EPS, p_no_outliers)
    p_no_outliers = min(1.0 - DBL_EPS, p_no_outliers)
    return log_probability / math.log(p_no_outliers)


class _Loop:
    """The state of RandomSampleConsensus::computeModel's loop and its step for one sample."""

    def __init__(self, pts, thr, probability, max_iterations):
        self.pts, self.thr, self.max_it = np.asarray(pts, F32), thr, max_iterations
        self.logp = math.log(1.0 - probability)
        self.best_count, self.best, self.best_coef = -INT_MAX, None, None
        self.iterations, self.skipped, self.k, self.done = 0, 0, 1.0, False
        self.hyp = []  # (triple, coef or None, count, status)

    def hypothesis(self, t):
        """(coef or None, count) of a sample: what a scoring launch computes ahead of the rule."""
        p = self.pts
        if collinear(p[t[0]], p[t[1]], p[t[2]]):
            return None, 0
        coef = plane_of(p[t[0]], p[t[1]], p[t[2]])
        return coef, int(within(coef, p, self.thr).sum())

    def step(self, t, coef, count):
        """The loop body for sample t (None: no sample could be selected)."""
        if t is None:
            self.done = True
            return
        self.hyp.append((tuple(int(v) for v in t), coef, count, 0 if coef is None else 1))
        if coef is None:  # computeModelCoefficients failed: skipped, not an iteration
            self.skipped += 1
            if self.skipped >= self.max_it * 10:
                self.done = True
            return
        if count > self.best_count:
            self.best_count, self.best, self.best_coef = count, tuple(int(v) for v in t), coef
            self.k = bound_k(count, len(self.pts), self.logp)
        self.iterations += 1
        if self.iterations > self.max_it:
            self.done = True
        if not (self.iterations < self.k):
            self.done = True

    def result(self):
        inl = np.flatnonzero(within(self.best_coef, self.pts, self.thr)) if self.best is not None else np.zeros(0, np.int64)
        return dict(sample=self.best, coef=self.best_coef, count=self.best_count if self.best is not None else 0,
                    iterations=self.iterations, skipped=self.skipped, k=self.k, inliers=inl, hypotheses=self.hyp)


def _source(pts, samples):
    if samples is None:
        return Sampler(pts).sample
    it = iter([tuple(int(v) for v in s) for s in samples])
    return lambda: next(it, None)


def ransac(pts, thr=0.1, probability=0.99, max_iterations=1000, samples=None):
    """pcl::RandomSampleConsensus::computeModel over SampleConsensusModelPlane, sequentially: sample, score, rule.
    samples: a list of triples in place of the sampler (the loop ends where the list does)."""
    loop, nxt = _Loop(pts, thr, probability, max_iterations), _source(pts, samples)
    while not loop.done:
        t = nxt()
        loop.step(t, *(loop.hypothesis(t) if t is not None else (None, 0)))
    return loop.result()


def ransac_batched(pts, batch, thr=0.1, probability=0.99, max_iterations=1000, samples=None):
    """The device's form: `batch` samples drawn ahead (the sampler never looks at a score), all of them scored, then the
    sequential rule replayed over the batch in order; what lies behind the end of the loop is dropped."""
    loop, nxt = _Loop(pts, thr, probability, max_iterations), _source(pts, samples)
    while not loop.done:
        ts = []
        for _ in range(batch):
            ts.append(nxt())
            if ts[-1] is None:
                break
        scored = [loop.hypothesis(t) if t is not None else (None, 0) for t in ts]
        for t, (coef, count) in zip(ts, scored):
            if loop.done:
                break
            loop.step(t, coef, count)
    return loop.result()


# ------------------------------------------------------------------------------------------------ the whole node
def detect(cloud, samples=None, batch=None, exact_nn=False, **params):
    """CloudFilter::DetectPlane over an (N, 4) cloud.  Returns a dict: found, reason, coeffs (f32 (4,) or None), the
    counts, iterations, skipped, k, winner (input indices), clip_org / normal_org (input index per point of the clipped /
    normal-filtered cloud), normals (the dict of `normals` over the clipped cloud, or None), keep, inliers (indices into
    the normal-filtered cloud), hypotheses, and the raw clouds normal_ground, ground, no_ground."""
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError(f"unknown ground parameter {k!r}")
        p[k] = v
    cloud = np.ascontiguousarray(np.asarray(cloud, F32)[:, :4])
    n = len(cloud)
    T, Ti = tilt_matrix(p["tilt_deg"])
    tilted = move(T, cloud)
    clip_org = np.flatnonzero(clip_mask(tilted, p["sensor_height"], p["height_clip_range"])) if n else np.zeros(0, np.int64)
    clipped = tilted[clip_org]
    nrm, keep = None, np.ones(len(clipped), bool)
    if p["use_normal_filtering"] and len(clipped):
        nrm = normals(clipped, p["normal_k"], p["sensor_height"], exact=exact_nn)
        keep = normal_keep(nrm["absz"], p["normal_filter_thresh"])
    normal_org = clip_org[keep]
    filtered = move(Ti, clipped[keep])
    empty = np.zeros((0, 4), F32)
    out = dict(found=False, reason="TOO_FEW_POINTS", coeffs=None, n_input=n, n_clipped=len(clipped), n_normal=len(filtered),
               n_inliers=0, iterations=0, skipped=0, k=1.0, winner=None, clip_org=clip_org, normal_org=normal_org, normals=nrm,
               keep=keep, inliers=np.zeros(0, np.int64), hypotheses=[], normal_ground=filtered, ground=empty, no_ground=empty)
    if len(filtered) < p["floor_pts_thresh"]:
        return out
    kw = dict(thr=p["ransac_threshold"], probability=p["ransac_probability"], max_iterations=p["ransac_max_iterations"],
              samples=samples)
    r = ransac(filtered, **kw) if batch is None else ransac_batched(filtered, batch, **kw)
    out.update(iterations=r["iterations"], skipped=r["skipped"], k=r["k"], hypotheses=r["hypotheses"], n_inliers=r["count"],
               winner=None if r["sample"] is None else tuple(int(normal_org[i]) for i in r["sample"]))
    if r["sample"] is None or len(r["inliers"]) < p["floor_pts_thresh"]:
        out["reason"] = "TOO_FEW_INLIERS"
        return out
    coef = r["coef"]
    ref = Ti[:3, 2]  # (T^-1 UnitZ).head3
    dot = (coef[0] * ref[0] + coef[1] * ref[1]) + coef[2] * ref[2]
    if abs(float(dot)) < math.cos(p["floor_normal_thresh"] * math.pi / 180.0):
        out["reason"] = "NOT_VERTICAL"
        return out
    if (coef[0] * F32(0) + coef[1] * F32(0)) + coef[2] * F32(1) < 0:  # make the normal upward
        coef = (coef * F32(-1)).astype(F32)
    inl = r["inliers"]
    gone = np.zeros(n, bool)
    # /no_ground_points: the input without the points the inliers came from, or the reference's form (:197-202), which
    # takes the inliers' indices in the filtered cloud for indices of the input cloud
    gone[inl if p["literal_no_ground"] else normal_org[inl]] = True
    out.update(found=True, reason="OK", coeffs=coef, inliers=inl, ground=filtered[inl], no_ground=cloud[~gone])
    return out
