"""decode_kernel + nms_kernel (detect.hip) and their host side (detector.cpp postprocess_chunk) on
planted head maps, against the restatement (oracle/scrfd.py detect_from_heads) of the same maps.

The whole-network tests only ever feed the post-processing a few dozen candidates with scores
near 0.606.  Here the head maps are written by hand (tests/_det_cases.py: what each case plants,
its preconditions and its candidate / survivor counts) and handed to the product's own
post-processing through frt_detector_postprocess.

Bars, the same for every case: counts equal; rows in the restatement's order; boxes and landmarks
bitwise equal (the kernels run the restatement's f32 operations in its order, detect.hip is compiled
with contraction off, division is correctly rounded); scores within 1e-6 (device expf against
np.exp; planted scores are >= 1e-5 apart, so the order never depends on it); rows of `dets` from
min(count, max_faces) on keep the NaN the wrapper filled them with.
"""
import numpy as np
import pytest

from tests import _det_cases as C
from tests import _frt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_recognition import FaceDetector
    return FaceDetector(state_dict=synthetic_detector_state_dict(), max_frames=4).model


def run(det, case, max_faces=256, frames=None, per_frame=None):
    """The case's frames (all, or `frames`) through the post-processing in calls of at most 4 frames.
    One scale for a call whose frames share it (the fr_detect form), per-frame scales otherwise (the
    fr_detect_images form); per_frame forces the choice."""
    frames = list(range(case.n)) if frames is None else list(frames)
    dets, counts = [], []
    for at in range(0, len(frames), 4):
        fs = frames[at:at + 4]
        heads = [h[fs] for h in case.heads]
        sc = case.scales[fs]
        ragged = bool((sc != sc[0]).any()) if per_frame is None else per_frame
        d, c = _frt.detector_postprocess(det, heads, det_scale=float(sc[0]), det_scales=sc if ragged else None,
                                         det_thresh=case.thresh, max_faces=max_faces)
        dets.append(d)
        counts.append(c)
    return np.concatenate(dets), np.concatenate(counts)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_frame(got, count, want, max_faces, what):
    """One frame's rows [max_faces][15] and count against the restatement's rows [k][15]."""
    assert count == len(want), (what, int(count), len(want))
    k = min(len(want), max_faces)
    g, w = got[:k], want[:k]
    box_lmk = [0, 1, 2, 3] + list(range(5, 15))
    same = (bits(g[:, box_lmk]) == bits(w[:, box_lmk])).all(axis=1)
    assert same.all(), (what, "first differing row", int(np.argmin(same)), g[np.argmin(same)], w[np.argmin(same)])
    if k:
        assert np.abs(g[:, 4] - w[:, 4]).max() <= 1e-6, what
    assert np.isnan(got[k:]).all(), (what, "rows beyond min(count, max_faces) were written")


def check(case, dets, counts, max_faces=256, frames=None):
    frames = list(range(case.n)) if frames is None else list(frames)
    assert len(counts) == len(frames)
    for i, f in enumerate(frames):
        check_frame(dets[i], counts[i], case.expected[f], max_faces, (case.name, f))


def test_empty(det):
    dets, counts = run(det, C.empty())
    assert counts.tolist() == [0] and np.isnan(dets).all()


@pytest.mark.parametrize("scale", [1.0, C.SCALE_1080P])
def test_level_ends(det, scale):
    """The first and last anchor of each level alone (flattened locations 0, 6399, 6400, 7999, 8000, 8399,
    both anchors: the loc -> level walk, anchor_base, the 2 + 4a / 10 + 10a channel offsets), distinct
    values in all 4 + 10 slots, then all twelve in one map."""
    case = C.level_ends(scale)
    check(case, *run(det, case))


@pytest.mark.parametrize("n", [1, 2, 3, 1024, 1025, 3000, 4096])
def test_sort_sizes(det, n):
    """Clustered candidates at every sort shape: no sort, one exchange, padding keys just above a power of
    two (3, 1025, 3000), one key per thread (1024), four keys per thread and no padding (4096)."""
    case = C.clustered(n)
    check(case, *run(det, case))


def test_over_the_candidate_limit(det):
    """4,097 candidates in frame 1 of two: FR_ERR_UNSUPPORTED naming the frame and the count; the handle
    then still serves the twelve-candidate map."""
    case = C.over_limit()
    with pytest.raises(NotImplementedError, match=r"frame 1 has 4097 anchors above det_thresh \(limit 4096\)"):
        run(det, case)
    again = C.twelve()
    check(again, *run(det, again))


def test_ties_order_by_anchor_and_repeat_bitwise(det):
    """Identical logits over all levels and anchors: decode_kernel's atomicAdd hands out slots in arrival
    order, the sort key (score desc, anchor asc) alone fixes the output (_det_cases.ties asserts that the
    expected rows ascend in anchor index inside a group).  Three calls give the same bits."""
    case = C.ties()
    runs = [run(det, case) for _ in range(3)]
    for dets, counts in runs:
        check(case, dets, counts)
    assert all(np.array_equal(bits(runs[0][0]), bits(d)) for d, _ in runs[1:])


def test_iou_exactly_at_the_threshold(det):
    case = C.iou_edge()
    check(case, *run(det, case))


def test_greedy_chain(det):
    case = C.greedy_chain()
    check(case, *run(det, case))


def test_score_exactly_at_the_threshold(det):
    case = C.score_at_threshold()
    check(case, *run(det, case))


@pytest.mark.parametrize("thresh", [0.3, 0.9])
def test_other_thresholds(det, thresh):
    case = C.clustered(1024, thresh)
    check(case, *run(det, case))


def test_per_frame_scales(det):
    """One map in four frames at four scales: each frame is the restatement at its own scale."""
    case = C.per_frame_scales()
    check(case, *run(det, case))
    # a uniform scale handed over per frame is the one-scale call
    one = C.clustered(300)
    a, b = run(det, one, per_frame=True), run(det, one, per_frame=False)
    check(one, *a)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_batch_independence(det):
    """Four different maps in one call: each frame's rows are what the frame gives when run alone."""
    case = C.mixed_batch()
    dets, counts = run(det, case)
    check(case, dets, counts)
    for f in range(case.n):
        d1, c1 = run(det, case, frames=[f], per_frame=True)
        assert c1[0] == counts[f] and np.array_equal(bits(d1[0]), bits(dets[f])), f


@pytest.mark.parametrize("max_faces", [0, 256, 1100, 2048, 4096])
def test_more_survivors_than_1024(det, max_faces):
    """1,100 disjoint boxes all survive: counts == 1100 and rows [0, min(1100, max_faces)) valid at every
    max_faces (include/frhip.h).  Before the device buffer was lifted to DET_MAX_CANDIDATES rows, rows
    1024.. came back unwritten at max_faces 1100, 2048 and 4096."""
    case = C.many_survivors()
    dets, counts = run(det, case, max_faces=max_faces)
    assert counts.tolist() == [1100]
    check(case, dets, counts, max_faces=max_faces)


def test_non_finite_and_degenerate_inputs(det):
    case = C.non_finite()
    check(case, *run(det, case))
