"""Inputs of the device quality gate's tests (tests/test_quality_gate_host.py on the CPU,
tests/test_gpu_quality_gate.py on the GPU) and the comparison rule both use.

``random_case``: seeded detections whose scores, box sizes and blur scores straddle the limits of
``FaceQualityFilter``'s defaults, with landmarks = the gate template of tests/_gate_inputs.py under
random roll, nose offsets and 0.4 px noise, laid out as frames of F slots with counts between 0 and
F.  ``planted_case``: the exact cases (values on a limit and one step off it, pitch exactly 30, a
zero roll, a NaN landmark, equal keys, a refused fit).
"""
import numpy as np

from tests._gate_inputs import _landmarks

OUTPUTS = ("stage", "metrics", "bbox", "rank", "rows", "frame_offsets", "valid_slots", "n_valid")
DEFAULTS = dict(min_det_score=0.6, min_face_size=60, max_yaw=45, max_pitch=30, max_roll=30, check_blur=True,
                blur_threshold=100)
PLANTED_CONFIG = dict(DEFAULTS, min_det_score=0.625)  # a limit that a float32 score can equal
SEED = 20260  # chosen so that test_quality_gate_host's precondition holds (it is asserted there)


def row_of(bbox, score, landmarks) -> np.ndarray:
    """One detection row: x0 y0 x1 y1 score, 5 x (x, y), float32 [15]."""
    return np.concatenate([np.asarray(bbox, np.float32), [np.float32(score)],
                           np.asarray(landmarks, np.float32).reshape(10)]).astype(np.float32)


def random_case(n_frames: int, F: int, seed: int = SEED):
    """-> (dets f32 [n,F,15], counts int32 [n], ok uint8 [n,F], blur f64 [n,F], planted) with
    ``planted`` the (frame, slots) groups given one key on purpose."""
    r = np.random.Generator(np.random.PCG64(seed))
    dets = np.zeros((n_frames, F, 15), np.float32)
    for f in range(n_frames):
        for i in range(F):
            scale = r.uniform(0.8, 1.5)
            lm = _landmarks(r.uniform(100, 800), r.uniform(100, 400), scale, r.uniform(-0.7, 0.7),
                            r.uniform(-20, 20), r.uniform(-20, 20)) + r.normal(0, 0.4, (5, 2)).astype(np.float32)
            x0, y0 = np.floor(lm.min(0)) - r.integers(0, 8, 2)
            w, h = r.integers(30, 90, 2)  # face_size = min(w, h) on both sides of 40 and 60
            dets[f, i] = row_of([x0 + r.uniform(0, 0.9), y0 + r.uniform(0, 0.9), x0 + w + r.uniform(0, 0.9),
                                 y0 + h + r.uniform(0, 0.9)], r.uniform(0.4, 1.0), lm)
    blur = r.uniform(0.0, 300.0, (n_frames, F))
    ok = (r.uniform(size=(n_frames, F)) > 0.15).astype(np.uint8)
    counts = r.integers(0, F + 1, n_frames).astype(np.int32)
    counts[0] = F
    planted = []
    if F >= 6:  # three slots of one key (one score, one blur) in the first frame
        slots = (1, 3, 4)
        for i in slots[1:]:
            dets[0, i, 4], blur[0, i] = dets[0, slots[0], 4], blur[0, slots[0]]
        planted.append((0, slots))
    return dets, counts, ok, blur, planted


def planted_case():
    """One frame of exact cases under ``PLANTED_CONFIG`` -> (dets [1,F,15], ok [1,F], blur [1,F], want)
    with ``want[i]`` the stage the slot must get."""
    base = _landmarks(300, 300, 1.2).astype(np.float32)  # a frontal face; its box is 100 x 120
    box = [240.0, 230.0, 340.9, 350.9]
    rows, ok, blur, want = [], [], [], []

    def add(stage, bbox=box, score=0.9, lm=base, fit=1, b=250.0):
        rows.append(row_of(bbox, score, lm))
        ok.append(fit)
        blur.append(b)
        want.append(stage)

    add(0, score=0.625)                                   # score == min_det_score: not below it
    add(1, score=np.nextafter(np.float32(0.625), np.float32(0)))
    add(0, bbox=[240.9, 230.2, 300.9, 350.0])             # face_size 60 == min_face_size
    add(2, bbox=[240.9, 230.2, 299.9, 350.0])             # 59
    # pitch exactly 30: (nose_y - eye_cy) == (mouth_cy - eye_cy) -> (1 - 0.5) * 60
    lm = base.copy()
    lm[0, 1] = lm[1, 1] = 256.0
    lm[3, 1] = lm[4, 1] = 320.0
    lm[2, 1] = 320.0
    add(0, lm=lm)
    lm2 = lm.copy()
    lm2[2, 1] = np.nextafter(np.float32(320.0), np.float32(1e9))  # one float32 step beyond: pitch > 30
    add(3, lm=lm2)
    lm3 = base.copy()
    lm3[1, 1] = lm3[0, 1]                                 # dy == 0: roll is exactly 0
    add(0, lm=lm3)
    lm4 = base.copy()
    lm4[2, 0] = np.nan                                    # a NaN nose_x: yaw NaN, which passes pose
    add(0, lm=lm4)
    for _ in range(3):                                    # three slots of one key: a stable order shows
        add(0, score=0.75, b=200.0)
    add(5, fit=0)                                         # passes every test, the fit was refused
    add(4, b=99.999)                                      # blur below the threshold
    add(1, score=0.3)
    return (np.stack(rows)[None], np.array(ok, np.uint8)[None], np.array(blur, np.float64)[None],
            np.array(want, np.uint8))


def ulps32(a, b) -> np.ndarray:
    """Distance in float32 steps between two arrays of float32-valued numbers (equal NaNs: 0)."""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.array_equal(a32.astype(np.float64), np.asarray(a, np.float64), equal_nan=True)
    ia, ib = a32.view(np.int32).astype(np.int64), b32.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    return np.where(np.isnan(a32) & np.isnan(b32), 0, np.where(np.isnan(a32) | np.isnan(b32), 1 << 40, d))


def assert_same_gate(got: dict, want: dict, what=""):
    """The rule between two statements of the gate that call different double atan2 / asin: every
    output bitwise, but yaw and roll (metrics columns 2 and 4) within one float32 ulp -- two double
    libraries agree to a few double ulp, so their float32 roundings differ only on a rounding
    boundary."""
    for k in OUTPUTS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if k != "metrics":
            assert np.array_equal(g, w), (what, k, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:8])
            continue
        for c in (0, 1, 3):
            assert np.array_equal(g[..., c].view(np.uint64), w[..., c].view(np.uint64)), (what, k, c)
        for c in (2, 4):
            u = ulps32(g[..., c], w[..., c])
            assert u.max(initial=0) <= 1, (what, k, c, int(u.max()))
