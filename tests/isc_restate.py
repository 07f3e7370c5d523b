"""Clean-room restatement of ISCGeneration (Intensity Scan Context, pgo_node's loop_method 2), written from
xchu_mapping/include/isc/ISCGeneration.cpp and its call sites in pgo_node.cpp — the oracle of tests/test_gpu_isc.py.

PARITY UNPINNED: the reference cannot be compiled here (no OpenCV, PCL or Eigen), so nothing checks this file against it.

Restated line by line (reference line numbers in the functions): ground_filter, calculate_isc, calculate_geometry_dis,
calculate_intensity_dis, is_loop_pair, makeAndSavedec, detectLoopClosureID, init_color.  The `*_literal` functions keep the
reference's loops; the vectorised ones used on whole routes are checked against them in tests/test_isc_restate.py.

Modelled: atan2f is (float)atan2((double)y, (double)x); Eigen's three-term sum is Eigen 3.3's SSE2 order, (x + y) + z.

Deviations from the reference, each where it leaves its row or depends on point order:
  1. a negative sector index (y = -0.0, x < 0: (float)pi > pi) is skipped; the reference writes in front of its row;
  2. outside the contract 0 <= intensity <= 1, (int)(255 * intensity) clamps to 0..255 and a NaN counts as 0; the
     reference's byte store wraps modulo 256 and then depends on point order;
  3. calculate_intensity_dis wraps its column with a true modulo; the reference subtracts `sectors` once and for
     angle >= sectors - 8 reads columns >= sectors (the next ring's cells, past the buffer on the last ring).
"""
import math

import numpy as np

RINGS, SECTORS, MAX_DIS = 60, 60, 40.0          # pgo_node.cpp:61-64
SKIP_NEIBOUR_DISTANCE = 20.0                    # ISCGeneration.h:36-43
INFLATION_COVARIANCE = 0.03
GEOMETRY_THRESHOLD = 0.67
INTENSITY_THRESHOLD = 0.91
Z_MIN, Z_MAX = np.float32(-0.9), np.float32(30.0)   # ground_filter (:289), PassThrough's f32 limits
WINDOW = 10


def color_table() -> np.ndarray:
    """init_color (:24-49): 272 entries in the listed order; cv::Vec3b's constructor takes uchar, so an int wraps."""
    t = [(0, i * 16, 255) for i in range(1)]
    t += [(0, i * 16, 255) for i in range(15)]
    t += [(0, 255, 255 - i * 16) for i in range(16)]
    t += [(i * 32, 255, 0) for i in range(32)]
    t += [(255, 255 - i * 16, 0) for i in range(16)]
    t += [(i * 4, 255, 0) for i in range(64)]
    t += [(255, 255 - i * 4, 0) for i in range(64)]
    t += [(255, i * 4, i * 4) for i in range(64)]
    return (np.array(t, np.int64) % 256).astype(np.uint8)


def ground_filter(cloud: np.ndarray) -> np.ndarray:
    """:284-291, PCL 1.7 PassThrough on z: non-finite points dropped, both limits inclusive."""
    c = np.asarray(cloud, np.float32).reshape(-1, 4)
    keep = np.isfinite(c[:, :3]).all(1) & (c[:, 2] >= Z_MIN) & (c[:, 2] <= Z_MAX)
    return c[keep]


def intensity_byte(w: np.ndarray) -> np.ndarray:
    v = np.float32(255) * np.asarray(w, np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.int32)   # truncation of a value in 0..255


def bin_ids(x, y, rings=RINGS, sectors=SECTORS, max_dis=MAX_DIS):
    """:69-79: (ring_id, sector_id, kept) of f32 coordinates."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    ring_step = max_dis / rings
    sector_step = 2 * math.pi / sectors
    distance = np.sqrt(x * x + y * y).astype(np.float64)               # f32 products, sum and root
    angle = math.pi + np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32).astype(np.float64)
    ring = np.floor(distance / ring_step)
    sector = np.floor(angle / sector_step)
    kept = (distance < max_dis) & (ring < rings) & (sector < sectors) & (sector >= 0)
    return ring.astype(np.int64), sector.astype(np.int64), kept


def calculate_isc(cloud: np.ndarray, rings=RINGS, sectors=SECTORS, max_dis=MAX_DIS) -> np.ndarray:
    """ground_filter + calculate_isc (:58-90): rings x sectors bytes, each cell its points' largest intensity byte."""
    c = ground_filter(cloud)
    ring, sector, kept = bin_ids(c[:, 0], c[:, 1], rings, sectors, max_dis)
    isc = np.zeros((rings, sectors), np.int32)
    np.maximum.at(isc, (ring[kept], sector[kept]), intensity_byte(c[kept, 3]))
    return isc.astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the two measures
def geometry_counts_literal(d1, d2):
    rings, sectors = d1.shape
    counts = []
    for i in range(sectors):
        match_count = 0
        for p in range(sectors):
            new_col = p + i - sectors if p + i >= sectors else p + i
            for q in range(rings):
                a, b = int(d1[q, p]), int(d2[q, new_col])
                if (a == 1 and b == 1) or (a == 0 and b == 0):     # "== true" / "== false" of a promoted byte
                    match_count += 1
        counts.append(match_count)
    return counts


def geometry_counts(d1, d2) -> np.ndarray:
    """match_count of every shift: the circular correlation of the "== 0" planes plus that of the "== 1" planes."""
    sectors = d1.shape[1]
    z = (d1 == 0).astype(np.int64).T @ (d2 == 0).astype(np.int64) + (d1 == 1).astype(np.int64).T @ (d2 == 1).astype(np.int64)
    p = np.arange(sectors)
    return np.array([z[p, (p + i) % sectors].sum() for i in range(sectors)], np.int64)


def first_max(counts):
    """:250-253: similarity starts at 0.0 and a strictly greater count replaces it; angle stays 0 when all are 0."""
    similarity, angle = 0, 0
    for i, c in enumerate(counts):
        if c > similarity:
            similarity, angle = int(c), i
    return similarity, angle


def calculate_geometry_dis(d1, d2, literal=False):
    """:231-257 -> (score, angle)."""
    rings, sectors = d1.shape
    similarity, angle = first_max(geometry_counts_literal(d1, d2) if literal else geometry_counts(d1, d2))
    return float(similarity) / (sectors * rings), angle


def intensity_sads(d1, d2, angle, literal=False):
    """SAD of the 20 shifts angle - 10 .. angle + 9 (:264-277), the column wrapped with a true modulo (deviation 3)."""
    rings, sectors = d1.shape
    out = []
    for i in range(angle - WINDOW, angle + WINDOW):
        if literal:
            s = 0
            for p in range(sectors):
                new_col = (p + i) % sectors
                for q in range(rings):
                    s += abs(int(d1[q, p]) - int(d2[q, new_col]))
        else:
            s = int(np.abs(d1.astype(np.int64) - np.roll(d2, -i, axis=1).astype(np.int64)).sum())
        out.append(s)
    return out


def calculate_intensity_dis(d1, d2, angle, literal=False):
    """:259-283."""
    rings, sectors = d1.shape
    difference = 1.0
    for s in intensity_sads(d1, d2, angle, literal):
        diff_temp = float(s) / (sectors * rings * 255)
        if diff_temp < difference:
            difference = diff_temp
    return 1 - difference


def is_loop_pair(d1, d2, geo_thres=GEOMETRY_THRESHOLD, inten_thres=INTENSITY_THRESHOLD):
    """:216-229 -> (is_loop, geo_score, inten_score, angle); inten_score stays 0 when the geometry does not pass."""
    geo, angle = calculate_geometry_dis(d1, d2)
    inten = 0.0
    if geo > geo_thres:
        inten = calculate_intensity_dis(d1, d2, angle)
        if inten > inten_thres:
            return True, geo, inten, angle
    return False, geo, inten, angle


def pair(d1, d2, geo_thres=GEOMETRY_THRESHOLD, inten_thres=INTENSITY_THRESHOLD):
    """What ndt_isc_pair reports: the intensity score computed whatever the geometry score is."""
    geo, angle = calculate_geometry_dis(d1, d2)
    inten = calculate_intensity_dis(d1, d2, angle)
    return geo, angle, inten, bool(geo > geo_thres and inten > inten_thres)


# ---------------------------------------------------------------------------------------------- the database
def narrow(pos):
    """pcl::PointXYZI holds the position in f32; Eigen::Vector3d widens it again (:201)."""
    return [float(np.float32(v)) for v in pos]


def distance3(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def gate(travel, pos, c, i, skip=SKIP_NEIBOUR_DISTANCE, inflation=INFLATION_COVARIANCE):
    """:165-169."""
    delta = travel[c] - travel[i]
    return delta > skip and distance3(pos[i], pos[c]) < delta * inflation


def detect_one(descs, pos, travel, c, cache=None, skip=SKIP_NEIBOUR_DISTANCE, inflation=INFLATION_COVARIANCE,
               geo_thres=GEOMETRY_THRESHOLD, inten_thres=INTENSITY_THRESHOLD) -> dict:
    """detectLoopClosureID (:157-193) with keyframe c as the newest; the record mirrors ndt_isc_result."""
    prev, best_score, best = 0, 0.0, (0.0, 0.0, 0)
    n_gated = n_geo = n_loop = 0
    for i in range(c + 1):
        if not gate(travel, pos, c, i, skip, inflation):
            continue
        n_gated += 1
        key = (c, i)
        if cache is not None and key in cache:
            ok, geo, inten, angle = cache[key]
        else:
            ok, geo, inten, angle = is_loop_pair(descs[c], descs[i], geo_thres, inten_thres)
            if cache is not None:
                cache[key] = (ok, geo, inten, angle)
        n_geo += geo > geo_thres
        if ok:
            n_loop += 1
            if geo + inten > best_score:
                best_score, prev, best = geo + inten, i, (geo, inten, angle)
    return {"loop_id": prev if prev != 0 else -1, "curr_id": c, "best_id": prev, "best_score": best_score, "geo_score": best[0],
            "inten_score": best[1], "angle": best[2], "n_gated": n_gated, "n_geometry": int(n_geo), "n_loop_pairs": n_loop}


def result_pair(rec):
    """The std::pair<int, float> the reference returns (:183-190)."""
    return (rec["loop_id"], np.float32(rec["curr_id"])) if rec["loop_id"] != -1 else (-1, np.float32(0.0))


class ISCGeneration:
    def __init__(self, rings=RINGS, sectors=SECTORS, max_dis=MAX_DIS, **thresholds):
        self.rings, self.sectors, self.max_dis = rings, sectors, max_dis
        self.thresholds = thresholds
        self.descs, self.pos, self.travel = [], [], []
        self.cache = {}
        self.last = None

    def add_descriptor(self, desc, pose_xyz):
        p = narrow(pose_xyz)
        self.travel.append(0.0 if not self.travel else self.travel[-1] + distance3(self.pos[-1], p))   # :204-211
        self.pos.append(p)
        self.descs.append(np.asarray(desc, np.uint8))
        return len(self.descs) - 1

    def makeAndSavedec(self, cloud, pose_xyz):
        return self.add_descriptor(calculate_isc(cloud, self.rings, self.sectors, self.max_dis), pose_xyz)

    def detect(self, c):
        return detect_one(self.descs, self.pos, self.travel, c, self.cache, **self.thresholds)

    def detectLoopClosureID(self):
        self.last = self.detect(len(self.descs) - 1)
        return result_pair(self.last)
