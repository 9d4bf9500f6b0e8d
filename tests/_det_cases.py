"""Planted head maps for the detector's post-processing (decode_kernel + nms_kernel), pure numpy.

A case is a set of SCRFD head maps written by hand -- logit -20 everywhere, candidates written in at
chosen (level, location, anchor) slots -- with the expected detections computed by the restatement
(oracle/scrfd.py detect_from_heads) on the same maps.  tests/test_gpu_det_postprocess.py runs the
maps through the product's post-processing (frt_detector_postprocess) and compares; test_detector.py
builds every case on the CPU, which runs the preconditions each builder asserts:

* distinct planted scores are at least 1e-5 apart, and at least 1e-5 from the threshold (a thousand
  times what device expf and np.exp can differ by), so neither the order nor the candidate set
  depends on the exponential; ties and the score-at-threshold case are planted as identical logit
  bits (logit +0.0 gives 0.5 exactly on both sides);
* the candidate and survivor counts are the ones the case is meant to have (EXPECTED_COUNTS).

Head layout per level: [n][h * w][32] = cls a0, cls a1 | bbox a0 (4), a1 (4) | kps a0 (10), a1 (10) |
2 zero pads, distances in stride units; levels 80x80 (stride 8), 40x40 (16), 20x20 (32).
"""
import functools

import numpy as np

from oracle import scrfd as R

STRIDES = (8, 16, 32)
SIDE = (80, 40, 20)
HW = (6400, 1600, 400)
ANCHOR_BASE = (0, 12800, 16000)
N_ANCHORS = 16800
BACKGROUND = np.float32(-20.0)
MAX_CANDIDATES = 4096      # DET_MAX_CANDIDATES
SCALE_1080P = 360 / 1080

# The score grid: 0.5 + (k + 1) * 1e-4, k < 4096, as f32 logits.
_P = 0.5 + (np.arange(4096, dtype=np.float64) + 1) * 1e-4
GRID_LOGITS = np.log(_P / (1 - _P)).astype(np.float32)


def sigmoid32(logit):
    """The f32 sigmoid expression of test_detector.py (and, up to expf, of decode_kernel)."""
    with np.errstate(all="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-logit))).astype(np.float32)


GRID_SCORES = sigmoid32(GRID_LOGITS)
assert np.all(np.diff(GRID_SCORES) >= 1e-5), "grid scores must be distinct, increasing, >= 1e-5 apart"


class Case:
    """heads: three arrays [n][hw][32]; scales: f32 [n]; expected[f]: f32 [k][15] rows in output order."""

    def __init__(self, name, heads, scales=1.0, thresh=0.5, exact_logits=()):
        self.name = name
        self.heads = heads
        self.n = heads[0].shape[0]
        self.scales = np.broadcast_to(np.asarray(scales, np.float32), (self.n,)).copy()
        self.thresh = float(np.float32(thresh))
        self.candidates, self.expected = [], []
        for f in range(self.n):
            logits = np.concatenate([h[f, :, 0:2].reshape(-1) for h in heads])
            scores = sigmoid32(logits)
            planted = np.isnan(logits) | (logits != BACKGROUND)
            _check_spacing(name, logits[planted], scores[planted], self.thresh, exact_logits)
            self.candidates.append(int(np.count_nonzero(scores >= np.float32(self.thresh))))
            self.expected.append(reference(heads, f, float(self.scales[f]), self.thresh)
                                 if self.candidates[-1] <= MAX_CANDIDATES else None)
        self.survivors = [None if e is None else len(e) for e in self.expected]
        for h in heads:
            h.setflags(write=False)
        want = EXPECTED_COUNTS.get(name)
        assert want is not None, f"{name}: add its counts to EXPECTED_COUNTS: {(self.candidates, self.survivors)}"
        assert (self.candidates, self.survivors) == want, (name, self.candidates, self.survivors, want)


def _check_spacing(name, logits, scores, thresh, exact_logits):
    """Distinct scores >= 1e-5 apart and from the threshold; equal scores only from equal logit bits."""
    ok = np.isfinite(scores)
    bits = logits[ok].view(np.uint32)
    uniq_bits, first = np.unique(bits, return_index=True)
    s = np.sort(scores[ok][first].astype(np.float64))
    if len(s) > 1:
        assert np.diff(s).min() >= 1e-5, (name, "planted scores closer than 1e-5", np.diff(s).min())
    exact = [np.float32(x).view(np.uint32) for x in exact_logits]
    near = [(b, v) for b, v in zip(bits[first], scores[ok][first]) if abs(float(v) - thresh) < 1e-5 and b not in exact]
    assert not near, (name, "a planted score within 1e-5 of the threshold", near[:3])


def reference(heads, f, det_scale, thresh):
    """The restatement's detections of frame f: [k][15] = x1 y1 x2 y2 score, 5 x (x, y), in output order."""
    sc, bb, kp = [], [], []
    for h in heads:
        m = h[f]
        sc.append(sigmoid32(m[:, 0:2].reshape(-1, 1)))
        bb.append(m[:, 2:10].reshape(-1, 4))
        kp.append(m[:, 10:30].reshape(-1, 10))
    with np.errstate(all="ignore"):
        det, kps = R.detect_from_heads(sc, bb, kp, det_scale, thresh)
    return np.hstack([det, kps.reshape(-1, 10)]).astype(np.float32)


def blank(n=1):
    heads = [np.zeros((n, hw, 32), np.float32) for hw in HW]
    for h in heads:
        h[:, :, 0:2] = BACKGROUND
    return heads


def put(heads, f, lv, loc, a, logit, dist, kps):
    """Write one candidate: dist (4) and kps (10) in stride units."""
    m = heads[lv][f, loc]
    assert m[a] == BACKGROUND, "slot already planted"
    m[a] = logit
    m[2 + 4 * a:6 + 4 * a] = dist
    m[10 + 10 * a:20 + 10 * a] = kps


def put_box(heads, f, lv, loc, a, logit, box, pts=None):
    """Write one candidate by its box (x1, y1, x2, y2) and 5 points in canvas pixels."""
    s = STRIDES[lv]
    ax, ay = (loc % SIDE[lv]) * s, (loc // SIDE[lv]) * s
    x1, y1, x2, y2 = box
    dist = np.array([ax - x1, ay - y1, x2 - ax, y2 - ay], np.float64) / s
    if pts is None:
        pts = [(x1 + (x2 - x1) * (k + 1) / 6, y1 + (y2 - y1) * (5 - k) / 6) for k in range(5)]
    kps = (np.asarray(pts, np.float64) - (ax, ay)).reshape(-1) / s
    put(heads, f, lv, loc, a, logit, dist.astype(np.float32), kps.astype(np.float32))


def slot(anchor):
    """Flattened anchor index -> (level, location, anchor of the location)."""
    lv = 2 if anchor >= ANCHOR_BASE[2] else 1 if anchor >= ANCHOR_BASE[1] else 0
    r = anchor - ANCHOR_BASE[lv]
    return lv, r // 2, r % 2


def anchor_of(case, f, rows):
    """The flattened anchor index of each expected row, found by its (unique) box among the planted slots."""
    out = []
    full = reference_all_boxes(case.heads, f, float(case.scales[f]))
    for r in rows:
        hit = np.flatnonzero((full.view(np.uint32) == r[:4].view(np.uint32)).all(axis=1))
        assert len(hit) == 1
        out.append(int(hit[0]))
    return out


def reference_all_boxes(heads, f, det_scale):
    sc = [np.ones((hw * 2, 1), np.float32) for hw in HW]
    bb = [h[f][:, 2:10].reshape(-1, 4) for h in heads]
    kp = [h[f][:, 10:30].reshape(-1, 10) for h in heads]
    with np.errstate(all="ignore"):
        _s, b, _k = R.decode(sc, bb, kp, 0.5)
    return (np.vstack(b) / np.float32(det_scale)).astype(np.float32)


# ------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def empty():
    return Case("empty", blank(1))


LEVEL_END_SLOTS = [(lv, loc, a) for lv in range(3) for loc in (0, HW[lv] - 1) for a in range(2)]


def _level_end_values(i):
    """Distinct distances in all 4 + 10 slots, distinct per candidate (multiples of 1/16: exact)."""
    dist = (np.arange(4) + 1) * 0.375 + i * 0.0625
    kps = (np.arange(10) - 4) * 0.1875 + i * 0.0625
    return dist.astype(np.float32), kps.astype(np.float32)


@functools.lru_cache(maxsize=None)
def level_ends(scale=1.0):
    """Frames 0..11: one candidate each at the first / last location of each level, both anchors (flattened
    locations 0, 6399, 6400, 7999, 8000, 8399); frame 12: all twelve."""
    heads = blank(13)
    for i, (lv, loc, a) in enumerate(LEVEL_END_SLOTS):
        dist, kps = _level_end_values(i)
        for f in (i, 12):
            put(heads, f, lv, loc, a, GRID_LOGITS[300 * i + 17], dist, kps)
    return Case(f"level_ends@{'1' if scale == 1.0 else '1080p'}", heads, scale)


@functools.lru_cache(maxsize=None)
def twelve():
    """The all-twelve map of level_ends alone (one frame)."""
    src = level_ends()
    return Case("twelve", [h[12:13].copy() for h in src.heads])


def _plant_clusters(heads, f, n, seed):
    """n candidates at n seeded slots, boxes jittered around 40 centres, scores a seeded permutation of
    the grid (without the grid point next to 0.9, a threshold the 1024-candidate map is run at)."""
    rng = np.random.default_rng(1000 + seed)
    perm = rng.permutation(4096)
    perm = perm[perm != 3999]
    perm = np.concatenate([perm, perm])           # more than 4095 candidates re-use scores (over-limit case)
    slots = rng.choice(N_ANCHORS, size=n, replace=False)
    centres = [(60 + 74 * i, 70 + 125 * j, 50 + 6 * ((3 * i + 5 * j) % 11)) for j in range(5) for i in range(8)]
    jit = rng.uniform(-0.3, 0.3, (n, 4))
    pj = rng.uniform(0.1, 0.9, (n, 5, 2))
    for i, an in enumerate(slots):
        lv, loc, a = slot(int(an))
        cx, cy, size = centres[i % 40]
        box = np.array([cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2]) + jit[i] * size
        pts = box[:2] + pj[i] * (box[2:] - box[:2])
        put_box(heads, f, lv, loc, a, GRID_LOGITS[perm[i]], box, pts)


@functools.lru_cache(maxsize=None)
def clustered(n, thresh=0.5, seed=0):
    heads = blank(1)
    _plant_clusters(heads, 0, n, seed)
    return Case(f"clustered{n}" + (f"@{thresh}" if thresh != 0.5 else "") + (f"#{seed}" if seed else ""), heads,
                thresh=thresh)


@functools.lru_cache(maxsize=None)
def over_limit():
    """Frame 0: the twelve-candidate map; frame 1: 4,097 candidates (a counted overflow: decode_kernel skips
    the slot past the limit, the host reports FR_ERR_UNSUPPORTED)."""
    heads = blank(2)
    for lv in range(3):
        heads[lv][0] = twelve().heads[lv][0]
    _plant_clusters(heads, 1, MAX_CANDIDATES + 1, 7)
    return Case("over_limit", heads)


@functools.lru_cache(maxsize=None)
def ties():
    """6 groups of 6 identical logits, a group's members on all three levels and both anchors, 20 px boxes
    on centres 100 px apart (disjoint: all 36 survive).  Expected order: score descending, then ascending
    flattened anchor index."""
    heads = blank(1)
    for g in range(6):
        for j in range(6):
            lv, a = j % 3, (j // 3 + g) % 2
            s = STRIDES[lv]
            # members in an order that is not the anchor order: columns run right to left
            gx, gy = round((50 + 100 * (5 - j)) / s), round((50 + 100 * g) / s)
            cx, cy = gx * s, gy * s
            put_box(heads, 0, lv, gy * SIDE[lv] + gx, a, GRID_LOGITS[500 * g + 100], (cx - 10, cy - 10, cx + 10, cy + 10))
    c = Case("ties", heads)
    rows = c.expected[0]
    an = anchor_of(c, 0, rows)
    for g in range(6):
        grp = slice(6 * g, 6 * g + 6)
        assert len(set(rows[grp, 4].view(np.uint32))) == 1, "a group is one score"
        assert an[grp] == sorted(an[grp]) and len({slot(x)[0] for x in an[grp]}) == 3
    return c


def _at(heads, f, loc, a, logit, box, origin):
    put_box(heads, f, 0, loc, a, logit, tuple(np.add(box, origin * 2)))


@functools.lru_cache(maxsize=None)
def iou_edge():
    """Integer boxes on the stride-8 level (distances in eighths, det_scale 1).  At (0, 0): areas 100 and
    40, intersection 40: IoU = f32(40 / 100) == f32(0.4), kept (ovr <= 0.4).  At (400, 400): the same pair
    with the second box one pixel taller (area 50, IoU 0.5): suppressed.  3 survivors of 4."""
    assert np.float32(40) / (np.float32(100) + np.float32(40) - np.float32(40)) == np.float32(0.4)
    heads = blank(1)
    L = GRID_LOGITS
    _at(heads, 0, 1 * 80 + 1, 0, L[4000], (0, 0, 9, 9), (0, 0))
    _at(heads, 0, 1 * 80 + 1, 1, L[3000], (0, 0, 9, 3), (0, 0))
    _at(heads, 0, 51 * 80 + 51, 0, L[2000], (0, 0, 9, 9), (400, 400))
    _at(heads, 0, 51 * 80 + 51, 1, L[1000], (0, 0, 9, 4), (400, 400))
    c = Case("iou_edge", heads)
    assert np.array_equal(c.expected[0][:, :4], np.array([[0, 0, 9, 9], [0, 0, 9, 3], [400, 400, 409, 409]], np.float32))
    return c


@functools.lru_cache(maxsize=None)
def greedy_chain():
    """A = x [0, 49], B = x [0, 99], C = x [50, 99], all y [0, 99], scores A > B > C.  IoU(A, B) = IoU(B, C)
    = 0.5, A and C do not overlap.  A suppresses B; B, suppressed, must not suppress C."""
    heads = blank(1)
    L = GRID_LOGITS
    o = (200, 200)
    _at(heads, 0, 25 * 80 + 25, 0, L[3000], (0, 0, 49, 99), o)
    _at(heads, 0, 25 * 80 + 25, 1, L[2000], (0, 0, 99, 99), o)
    _at(heads, 0, 25 * 80 + 26, 0, L[1000], (50, 0, 99, 99), o)
    c = Case("greedy_chain", heads)
    assert np.array_equal(c.expected[0][:, :4], np.array([[200, 200, 249, 299], [250, 200, 299, 299]], np.float32))
    return c


@functools.lru_cache(maxsize=None)
def score_at_threshold():
    """Logit +0.0: score 0.5 exactly (exp(-0) == 1), kept at det_thresh 0.5; two grid scores beside it."""
    heads = blank(1)
    put_box(heads, 0, 0, 10 * 80 + 10, 0, np.float32(0.0), (70, 70, 95, 95))
    put_box(heads, 0, 1, 20 * 40 + 20, 1, GRID_LOGITS[10], (300, 300, 340, 340))
    put_box(heads, 0, 2, 15 * 20 + 3, 0, GRID_LOGITS[900], (80, 460, 140, 520))
    c = Case("score_at_threshold", heads, exact_logits=(0.0,))
    assert c.expected[0][2, 4] == np.float32(0.5)
    return c


FRAME_SCALES = (1.0, SCALE_1080P, 640 / 1080, 2.5)


@functools.lru_cache(maxsize=None)
def per_frame_scales():
    """The same clustered map in four frames at four scales (the +1 of the box areas makes NMS depend on it)."""
    one = clustered(300).heads
    return Case("per_frame_scales", [np.repeat(h, 4, axis=0) for h in one], FRAME_SCALES)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Four different maps in one call, each at its own scale."""
    parts = [clustered(300, seed=1), twelve(), ties(), greedy_chain()]
    return Case("mixed_batch", [np.concatenate([p.heads[lv] for p in parts]) for lv in range(3)],
                (SCALE_1080P, 1.0, 0.5, 1.0))


@functools.lru_cache(maxsize=None)
def many_survivors():
    """1,100 disjoint candidates: the first 1,100 locations of the stride-8 level, anchor 0, distances 0.25
    (5 px boxes on 8 px centres).  More survivors than the 1,024 rows the device buffer used to hold."""
    heads = blank(1)
    perm = np.random.default_rng(5).permutation(4096)[:1100]
    dist = np.full(4, 0.25, np.float32)
    for i in range(1100):
        put(heads, 0, 0, i, 0, GRID_LOGITS[perm[i]], dist, ((np.arange(10) % 3 - 1) * 0.125).astype(np.float32))
    return Case("many_survivors", heads)


@functools.lru_cache(maxsize=None)
def non_finite():
    """A NaN logit (dropped: NaN >= t is false), a +inf logit (score 1, first), a box with x2 < x1, a
    low-ranked box with a NaN coordinate (its overlap with the first pivot is NaN: not `<= t`, removed),
    among ordinary boxes."""
    heads = blank(1)
    L = GRID_LOGITS
    put_box(heads, 0, 0, 30 * 80 + 30, 0, np.float32(np.nan), (230, 230, 260, 260))
    put_box(heads, 0, 0, 40 * 80 + 40, 0, np.float32(np.inf), (300, 300, 350, 350))
    put_box(heads, 0, 0, 40 * 80 + 41, 1, L[3500], (310, 305, 352, 349))      # suppressed by the +inf box
    put_box(heads, 0, 1, 10 * 40 + 10, 0, L[3000], (170, 150, 150, 180))      # x2 < x1
    put_box(heads, 0, 1, 10 * 40 + 10, 1, L[2500], (140, 140, 185, 185))      # around the inverted box
    put_box(heads, 0, 2, 5 * 20 + 15, 0, L[2000], (450, 130, 520, 200))
    put_box(heads, 0, 2, 5 * 20 + 15, 1, L[100], (np.nan, 500, 560, 560))     # NaN x1, low rank
    put_box(heads, 0, 0, 70 * 80 + 70, 1, L[50], (550, 550, 580, 580))
    c = Case("non_finite", heads)
    assert c.expected[0][0, 4] == np.float32(1.0) and np.isfinite(c.expected[0]).all()
    return c


# (candidates per frame, survivors per frame) as the restatement computes them; None: over the limit.
EXPECTED_COUNTS = {
    "empty": ([0], [0]),
    "level_ends@1": ([1] * 12 + [12], [1] * 12 + [6]),
    "level_ends@1080p": ([1] * 12 + [12], [1] * 12 + [6]),
    "twelve": ([12], [6]),
    "clustered1": ([1], [1]),
    "clustered2": ([2], [2]),
    "clustered3": ([3], [3]),
    "clustered1024": ([1024], [113]),
    "clustered1025": ([1025], [113]),
    "clustered3000": ([3000], [143]),
    "clustered4096": ([4096], [155]),
    "over_limit": ([12, 4097], [6, None]),
    "ties": ([36], [36]),
    "iou_edge": ([4], [3]),
    "greedy_chain": ([3], [2]),
    "score_at_threshold": ([3], [3]),
    "clustered1024@0.3": ([1024], [113]),
    "clustered1024@0.9": ([27], [22]),
    "clustered300": ([300], [85]),
    "clustered300#1": ([300], [85]),
    "per_frame_scales": ([300] * 4, [85, 87, 87, 85]),
    "mixed_batch": ([300, 12, 36, 3], [88, 6, 36, 2]),
    "many_survivors": ([1100], [1100]),
    "non_finite": ([7], [5]),
}


def all_cases():
    """Every case the GPU tests run (building one runs its preconditions)."""
    out = [empty(), level_ends(1.0), level_ends(SCALE_1080P), twelve()]
    out += [clustered(n) for n in (1, 2, 3, 1024, 1025, 3000, 4096)]
    out += [over_limit(), ties(), iou_edge(), greedy_chain(), score_at_threshold(), clustered(1024, 0.3),
            clustered(1024, 0.9), per_frame_scales(), mixed_batch(), many_survivors(), non_finite()]
    return out
