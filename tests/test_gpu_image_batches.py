"""Mixed-size image batches: ``fr_detect_images`` / ``fr_align_images`` (one detect call and one align
launch over n images of n sizes) and what stands on them -- ``FaceDetector.detect_images``,
``FaceAligner.align_images``, ``FaceProcessor.process_images`` and ``DatasetPreprocessor``.

Per image the batch is the single-image path: the letterboxed canvas bit for bit, the head maps to
fp32 rounding (the network runs in another batch and, in a mixed chunk, under another row plan),
decode with the image's own scale, crops and transforms bit for bit.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import scrfd as R
from tests import _frt
from tests.test_gpu_detector_rows import _frames

pytestmark = pytest.mark.gpu

SIZES = [(1080, 1920), (481, 367), (37, 53), (640, 640),
         (720, 1280), (600, 1400), (1, 1), (2, 3),
         (333, 1001)]
MAX_FRAMES = 4
CHUNKS = [range(0, 4), range(4, 8), range(8, 9)]


@pytest.fixture(scope="module")
def det():
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_recognition import FaceDetector
    return FaceDetector(state_dict=synthetic_detector_state_dict(), max_frames=MAX_FRAMES)


@pytest.fixture(scope="module")
def images():
    return [_frames(sum(s) + i, 1, *s)[0].contiguous() for i, s in enumerate(SIZES)]


def _forward_images(handle, imgs):
    """frt_detector_forward_images: one chunk's head maps and full canvases."""
    from facerecognitionpipeline_amd import _lib
    L = _lib.load()
    L.frt_detector_forward_images.restype = ctypes.c_int
    L.frt_detector_forward_images.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    kept, ptrs, sizes = handle._image_list(imgs)
    n = len(kept)
    levels = [(640 // s, 640 // s) for s in (8, 16, 32)]
    heads = torch.empty(sum(n * h * w * 32 for h, w in levels), dtype=torch.float32, device=kept[0].device)
    canvas = torch.empty((n, 640, 640, 3), dtype=torch.uint8, device=kept[0].device)
    rc = L.frt_detector_forward_images(handle.h, ptrs.ctypes.data, sizes.ctypes.data, n, heads.data_ptr(),
                                       canvas.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, handle.h)
    out, off = [], 0
    for h, w in levels:
        out.append(heads[off:off + n * h * w * 32].view(n, h, w, 32).cpu().numpy())
        off += n * h * w * 32
    return out, canvas.cpu().numpy()


@pytest.fixture(scope="module")
def chunk_runs(det, images):
    """Per chunk of the 9-image call: (head maps per level, canvases), run as fr_detect_images runs it."""
    return [_forward_images(det.model, [images[i] for i in c]) for c in CHUNKS]


@pytest.fixture(scope="module")
def all_dets(det, images):
    return det.model.detect_images(images, 0.5, 1024)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_reduction", [1, 0])
def test_same_size_equals_fr_detect(det, row_reduction):
    frames = _frames(2000, 3, 720, 1280)
    try:
        _frt.set_detector_row_reduction(det.model, row_reduction)
        d_img, c_img = det.model.detect_images([frames[i] for i in range(3)], 0.5, 256)
        d_ref, c_ref = det.model.detect(frames, 0.5, 256)
    finally:
        _frt.set_detector_row_reduction(det.model, 1)
    assert c_ref.min() > 0
    assert np.array_equal(c_img, c_ref)
    assert d_img.tobytes() == d_ref.tobytes()


# 2 ------------------------------------------------------------------------------------------------
def test_canvas_is_the_single_image_letterbox(images, chunk_runs):
    for c, (_heads, canvas) in zip(CHUNKS, chunk_runs):
        for b, i in enumerate(c):
            want, _ = R.letterbox(images[i].cpu().numpy())
            assert np.array_equal(canvas[b], want), SIZES[i]


# 3 ------------------------------------------------------------------------------------------------
def test_heads_match_each_image_alone(det, images, chunk_runs):
    """frt_detector_forward takes sides from 2, as fr_detect does; the 1x1 image alone goes through
    frt_detector_forward_images as a chunk of one (its own geometry and row plan, batch 1)."""
    worst = 0.0
    ratios = {}
    for c, (heads, _canvas) in zip(CHUNKS, chunk_runs):
        for b, i in enumerate(c):
            if min(SIZES[i]) >= 2:
                alone = [x[0].cpu().numpy() for x in _frt.detector_forward(det.model, images[i][None])[0]]
            else:
                alone = [x[0] for x in _forward_images(det.model, [images[i]])[0]]
            for lv in range(3):
                a = alone[lv]
                ratio = float(np.abs(a - heads[lv][b]).max() / np.abs(a).max())
                ratios[(SIZES[i], lv)] = ratio
                worst = max(worst, ratio)
    print("largest max|chunk - alone| / max|alone| over images and levels: %.3e" % worst)
    for key, ratio in ratios.items():
        assert ratio <= 1e-5, (key, ratio)


# 4 ------------------------------------------------------------------------------------------------
TIE_GAP = 3e-7  # about 5 ulp of a score in [0.5, 1): see _order_sensitive


def _order_sensitive(cand, logits):
    """Whether the reference's own result turns on the order of two candidates it cannot tell apart:
    cand is the reference's pre-NMS list ([x1 y1 x2 y2 score | landmarks], already / det_scale); two
    neighbours of its sorted order that come from different logits and score within TIE_GAP are
    swapped, and NMS is run again.  True when some swap changes the kept list (another box kept, or
    two kept boxes trade places); swaps of candidates that a stronger box suppresses anyway change
    nothing and do not count.

    Equal logits give equal scores on the device and in numpy alike, and both break that tie by anchor
    index, so such pairs are no hazard.  Different logits go through two exponentials: the device's
    expf and numpy's exp are each good to an ulp or two of exp(-x), the sigmoid halves that relative
    error for a score >= 0.5 and the add and the divide round once each, so a score carries up to about
    2.5 ulp and a pair closer than about 5 ulp (5 * 2^-24 = 3e-7, TIE_GAP) may sort either way."""
    n = cand.shape[0]
    order = np.lexsort((np.arange(n), -cand[:, 4].astype(np.float64)))  # detect_from_heads' order
    rows, lg = cand[order], logits[order]
    kept = np.delete(rows[R._nms_sorted(rows[:, :5])], 4, axis=1)
    for p in range(n - 1):
        if lg[p] != lg[p + 1] and float(rows[p, 4]) - float(rows[p + 1, 4]) <= TIE_GAP:
            sw = rows.copy()
            sw[[p, p + 1]] = sw[[p + 1, p]]
            other = np.delete(sw[R._nms_sorted(sw[:, :5])], 4, axis=1)
            if not np.array_equal(other, kept):
                return True
    return False


def test_decode_uses_each_images_scale(images, chunk_runs, all_dets):
    """The pattern of test_detector.test_detections_match_postprocessing_of_gpu_heads for every image of
    the nine-image call, with the image's own letterbox scale: counts equal, scores within 1e-6, boxes
    and landmarks bitwise equal, in the reference's order.

    The exception is an image in which the reference's own result turns on a tie: swapping two
    candidates of different logits within TIE_GAP in score changes what its NMS keeps (_order_sensitive,
    decided from the reference's candidates alone).  The device's expf and numpy's exp may order such
    a pair differently, and NMS then keeps the other member of the cluster.  Seen on the GPU for 37x53, which is upscaled twelve times into flat
    blocks whose anchors score equal to the last bit: position 32 of 55, four candidates within 1e-6, the
    nearest 2.65 px away.  Such an image is held to the same count, the same scores in order within
    1e-6, and every detection's boxes and landmarks equal to a reference pre-NMS candidate of its score (within
    1e-6), decoded with this image's scale, one to one.  Images of at least two scales must take the
    ordered comparison."""
    dets, counts = all_dets
    ordered, tied = [], []
    for c, (heads, _canvas) in zip(CHUNKS, chunk_runs):
        for b, i in enumerate(c):
            sc, bb, kp = [], [], []
            for lv in range(3):
                h = heads[lv][b].reshape(-1, 32)
                logit = h[:, 0:2].reshape(-1, 1)
                sc.append((np.float32(1) / (np.float32(1) + np.exp(-logit))).astype(np.float32))
                bb.append(h[:, 2:10].reshape(-1, 4))
                kp.append(h[:, 10:30].reshape(-1, 10))
            scale = R.letterbox_geometry(*SIZES[i])[2]
            want, wkps = R.detect_from_heads(sc, bb, kp, scale, 0.5)
            n = int(counts[i])
            assert n == len(want) and n > 0, (SIZES[i], n, len(want))
            got = dets[i, :n]
            assert np.abs(got[:, 4] - want[:, 4]).max() <= 1e-6, SIZES[i]
            # the reference's candidates before NMS: [x1 y1 x2 y2 score | 5 x (x, y)] / this image's scale
            s_l, b_l, k_l = R.decode(sc, bb, kp, 0.5)
            cand = np.concatenate([(np.vstack(b_l) / np.float32(scale)).astype(np.float32), np.vstack(s_l),
                                   (np.vstack(k_l).reshape(-1, 10) / np.float32(scale)).astype(np.float32)], axis=1)
            logits = np.concatenate([heads[lv][b].reshape(-1, 32)[:, 0:2].reshape(-1)[sc[lv].reshape(-1) >= 0.5]
                                     for lv in range(3)])
            assert logits.shape[0] == cand.shape[0]
            if not _order_sensitive(cand, logits):
                assert np.array_equal(got[:, :4].view(np.uint32), want[:, :4].view(np.uint32)), SIZES[i]
                assert np.array_equal(np.ascontiguousarray(got[:, 5:]).view(np.uint32),
                                      np.ascontiguousarray(wkps.reshape(-1, 10)).view(np.uint32)), SIZES[i]
                ordered.append(SIZES[i])
                continue
            tied.append(SIZES[i])
            used = np.zeros(len(cand), bool)
            for p, g in enumerate(got):
                near = np.where(~used & (np.abs(cand[:, 4] - g[4]) <= 1e-6))[0]
                assert near.size, (SIZES[i], p)
                err = np.abs(np.delete(cand[near], 4, axis=1) - np.delete(g, 4)).max(axis=1)
                assert err.min() == 0, (SIZES[i], p, float(err.min()))
                used[near[int(err.argmin())]] = True
    print("ordered comparison asserted for:", ordered, "tie in the reference, candidates matched for:", tied)
    assert len({R.letterbox_geometry(*s)[2] for s in ordered}) >= 2, (ordered, tied)


# 5 ------------------------------------------------------------------------------------------------
def test_chunk_seam_and_order(det, images, all_dets):
    dets, counts = all_dets
    for c in CHUNKS:
        d, n = det.model.detect_images([images[i] for i in c], 0.5, 1024)
        for b, i in enumerate(c):
            assert n[b] == counts[i] and d[b].tobytes() == dets[i].tobytes(), SIZES[i]
    rev = images[::-1]
    d_rev, n_rev = det.model.detect_images(rev, 0.5, 1024)
    for at in range(0, len(rev), MAX_FRAMES):
        d, n = det.model.detect_images(rev[at:at + MAX_FRAMES], 0.5, 1024)
        assert np.array_equal(n, n_rev[at:at + MAX_FRAMES])
        assert d.tobytes() == d_rev[at:at + MAX_FRAMES].tobytes(), at


# 6 ------------------------------------------------------------------------------------------------
def _landmarks(r, H, W, k, S=112):
    """k faces' landmarks: the template under a random similarity, centred anywhere from outside the
    image's border to inside it (so crops read partly, or wholly, outside the image)."""
    t = np.array([[0.34, 0.46], [0.66, 0.46], [0.50, 0.61], [0.37, 0.74], [0.63, 0.74]]) * S - S / 2
    out = np.empty((k, 5, 2), np.float32)
    for j in range(k):
        a, sc = r.uniform(-0.6, 0.6), r.uniform(0.05, 1.5) * max(min(H, W), 8) / S
        rot = sc * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        centre = (r.uniform(-0.1 * W - 4, 1.1 * W + 4), r.uniform(-0.1 * H - 4, 1.1 * H + 4))
        out[j] = (t @ rot.T + centre + r.normal(0, 0.3, (5, 2))).astype(np.float32)
    return out


@pytest.mark.parametrize("S", [112, 224])
def test_align_images_is_align_faces_per_image(S):
    from facerecognitionpipeline_amd.face_recognition import FaceAligner
    al = FaceAligner(output_size=S)
    h = al._ops.handle
    r = np.random.default_rng(60 + S)
    sizes = [(1080, 1920), (37, 53), (481, 367), (5, 9), (640, 640)]
    faces = [21, 13, 0, 9, 12]  # 55 faces (> the 48 maps fr_warp_affine passes by value), one image without
    imgs = [torch.from_numpy(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for H, W in sizes]
    lms = [_landmarks(r, H, W, k) for (H, W), k in zip(sizes, faces)]
    want, want_tf = [], []
    for im, lm in zip(imgs, lms):
        out = torch.empty((lm.shape[0], S, S, 3), dtype=torch.uint8, device=im.device)
        if lm.shape[0]:
            want_tf.append(h.align_faces(im, lm, S, out))
        want.append(out)
    want, want_tf = torch.cat(want).cpu().numpy(), np.concatenate(want_tf)
    assert want.shape[0] == 55 and (want.reshape(55, -1) == 0).all(axis=1).sum() < 28  # most crops have content
    face_image = np.repeat(np.arange(5, dtype=np.int32), faces)
    lm_all = np.concatenate(lms)
    got = torch.empty((55, S, S, 3), dtype=torch.uint8, device=imgs[0].device)
    tf = h.align_images(imgs, lm_all, face_image, S, got)
    assert np.array_equal(got.cpu().numpy(), want)
    assert tf.tobytes() == want_tf.tobytes()
    assert np.array_equal(al.align_images(imgs, lms).cpu().numpy(), want)        # the public form
    assert np.array_equal(al.align_images([x.cpu().numpy() for x in imgs], lms).cpu().numpy(), want)
    perm = r.permutation(55)                                                     # faces in any order
    got.zero_()
    tf = h.align_images(imgs, lm_all[perm], face_image[perm], S, got)
    assert np.array_equal(got.cpu().numpy(), want[perm]) and tf.tobytes() == want_tf[perm].tobytes()


def test_align_images_other_methods_run_per_image():
    from facerecognitionpipeline_amd.face_recognition import FaceAligner
    al = FaceAligner(output_size=112)
    r = np.random.default_rng(7)
    imgs = [torch.from_numpy(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for H, W in ((90, 120), (200, 150))]
    lms = [_landmarks(r, 90, 120, 2), _landmarks(r, 200, 150, 3)]
    got = al.align_images(imgs, lms, method="affine")
    want = torch.cat([al.align_batch(im, lm, "affine") for im, lm in zip(imgs, lms)])
    assert torch.equal(got, want) and got.shape[0] == 5


# 7 ------------------------------------------------------------------------------------------------
def test_arguments(det):
    from facerecognitionpipeline_amd import _lib
    from facerecognitionpipeline_amd.face_recognition import FaceAligner
    m = det.model
    ok = torch.zeros((40, 50, 3), dtype=torch.uint8, device="cuda")
    d, c = m.detect_images([], 0.5, 256)
    assert d.shape == (0, 256, 15) and c.shape == (0,)
    d, c = m.detect_images([ok], 0.5, 256)                                       # a list of one image
    assert d.shape == (1, 256, 15) and c.shape == (1,)
    assert det.detect_images([]) == [] and len(det.detect_images([ok.cpu().numpy()[:, :, 0]])) == 1  # gray
    with pytest.raises(ValueError, match="image 2"):                             # a NULL pointer
        m.detect_images([ok, ok, torch.zeros((0, 50, 3), dtype=torch.uint8, device="cuda")], 0.5, 256)
    with pytest.raises(ValueError, match="image 1 .*8193"):                      # a side outside [1, 8192]
        m.detect_images([ok, torch.zeros((8193, 1, 3), dtype=torch.uint8, device="cuda")], 0.5, 256)
    with pytest.raises(ValueError, match="image 1 is too small to letterbox"):
        m.detect_images([ok, torch.zeros((1, 700, 3), dtype=torch.uint8, device="cuda")], 0.5, 256)
    with pytest.raises(ValueError, match="max_faces"):
        m.detect_images([ok], 0.5, 0)
    for bad in (ok.float(), ok[:, :, :2], ok[0]):
        with pytest.raises(ValueError):
            m.detect_images([bad], 0.5, 256)
    # fr_align_images (any handle: the detector's will do)
    al = FaceAligner(output_size=112)
    lm = _landmarks(np.random.default_rng(1), 40, 50, 2)
    out = torch.empty((2, 112, 112, 3), dtype=torch.uint8, device="cuda")
    assert m.align_images([ok, ok], lm, [1, 0], 112, out).shape == (2, 2, 3)
    for fi in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="names image"):
            m.align_images([ok, ok], lm, fi, 112, out)
    with pytest.raises(ValueError):
        m.align_images([ok], lm, [0, 0], 0, torch.empty((2, 0, 0, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):                                              # out of another shape
        m.align_images([ok], lm, [0, 0], 112, out[:1])
    with pytest.raises(ValueError):                                              # faces without an image each
        m.align_images([ok], lm, [0], 112, out)
    L = _lib.load()
    kept, ptrs, sizes = m._image_list([ok])
    fi = np.zeros(2, np.int32)
    rc = L.fr_align_images(m.h, ptrs.ctypes.data, sizes.ctypes.data, 1, lm.ctypes.data, fi.ctypes.data, 2, 112,
                           None, None, torch.cuda.current_stream().cuda_stream)   # NULL out
    assert rc == _lib.FR_ERR_INVALID_ARGUMENT
    empty = torch.empty((0, 112, 112, 3), dtype=torch.uint8, device="cuda")
    assert m.align_images([ok], np.zeros((0, 5, 2), np.float32), [], 112, empty).shape == (0, 2, 3)
    assert m.align_images([], np.zeros((0, 5, 2), np.float32), [], 112, empty).shape == (0, 2, 3)
    assert al.align_images([], []).shape == (0, 112, 112, 3)
    assert al.align_images([ok], [np.zeros((0, 5, 2), np.float32)]).shape == (0, 112, 112, 3)


# 8 ------------------------------------------------------------------------------------------------
class FixedDetector:
    """The reference detector's contract with fixed answers: a few faces per image, placed by its size
    (none for the smallest), det scores on both sides of the gate."""

    def detect(self, image):
        H, W = image.shape[:2]
        r = np.random.default_rng(H * 10007 + W)
        k = 0 if min(H, W) < 50 else 3 + (H + W) % 4
        lm = _landmarks(r, H, W, k)
        out = []
        for j in range(k):
            lo, hi = lm[j].min(0), lm[j].max(0)
            out.append({"bbox": np.array([lo[0] - 10, lo[1] - 20, hi[0] + 10, hi[1] + 10]).astype(np.int32),
                        "landmarks": lm[j], "det_score": float(r.uniform(0.4, 1.0)), "pose": None, "age": None,
                        "gender": None})
        return out


def _mixed_images():
    r = np.random.default_rng(88)
    out = []
    for i, (H, W) in enumerate([(540, 960), (333, 250), (40, 30), (300, 420)]):
        im = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
        im[: H // 2] = (np.arange(W)[None, :, None] // 5 % 256).astype(np.uint8)  # a smooth half: low blur scores
        out.append(im)
    out[3] = np.ascontiguousarray(out[3][:, :, 1])  # a gray 2-D image
    return out


def _same_result(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        elif isinstance(a[k], dict):
            assert list(a[k]) == list(b[k]), k
            for q in a[k]:
                assert type(a[k][q]) is type(b[k][q]) and a[k][q] == b[k][q], (k, q)
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


@pytest.mark.parametrize("return_all", [False, True])
def test_process_images_equals_process_numpy_with_fixed_detections(return_all):
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    fp = FaceProcessor(output_size=112, detector=FixedDetector(),
                       quality_filter_config={"min_det_score": 0.5, "min_face_size": 20})
    imgs = _mixed_images()
    got = fp.process_images(imgs, return_all)
    want = [fp.process_numpy(im, return_all) for im in imgs]
    assert [len(x) for x in got] == [len(x) for x in want] and got[2] == []
    assert sum(len(x) for x in want) >= (10 if return_all else 1)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            _same_result(a, b)
    if return_all:
        assert got[3][0]["aligned_face"].ndim == 2
        assert {r["is_valid"] for x in want for r in x} == {True, False}


def test_process_images_reports_bad_items(tmp_path):
    from PIL import Image
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    fp = FaceProcessor(output_size=112, detector=FixedDetector(), quality_filter_config={"min_face_size": 0})
    imgs = _mixed_images()
    good = str(tmp_path / "good.png")
    Image.fromarray(imgs[0]).save(good)
    bad = str(tmp_path / "bad.png")
    with open(bad, "wb") as f:
        f.write(b"no image")
    with pytest.raises(ValueError, match="Could not load image"):
        fp.process_images([imgs[1], bad, good], True)
    out = fp.process_images([imgs[1], bad, good, np.zeros((4, 4, 2), np.uint8)], True, errors="return")
    assert isinstance(out[1], ValueError) and isinstance(out[3], ValueError)
    for a, b in zip(out[2], fp.process_image(good, True)):
        _same_result(a, b)
    for a, b in zip(out[0], fp.process_numpy(imgs[1], True)):
        _same_result(a, b)
    assert fp.process_images([], True) == []


def _noise(seed, H, W):
    """A frame of noise, as test_detector._frame: no smooth region.  (The smooth third of
    test_gpu_detector_rows._frames gives clusters of anchors with equal scores; which member NMS keeps
    then turns on the last bit of a score, so the single-image and the batched run -- the same
    network in another batch, 5e-7 apart -- may keep neighbours 12 px apart.  Detections of distinct
    scores are what the 1 px bound is about.)"""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _match_faces(got, want):
    """Every face of ``got`` has its face in ``want``: det_score within 1e-5, box within 1 px (the int
    cast of a box may flip on a 1e-3 difference; near-equal scores may trade places in the order)."""
    assert len(got) == len(want)
    left = list(range(len(want)))
    for g in got:
        j = min(left, key=lambda j: np.abs(want[j]["bbox"].astype(np.int64) - g["bbox"]).max())
        assert np.abs(want[j]["bbox"].astype(np.int64) - g["bbox"]).max() <= 1, (g["bbox"], want[j]["bbox"])
        assert abs(want[j]["det_score"] - g["det_score"]) <= 1e-5
        left.remove(j)


def test_process_images_with_the_gpu_detector(det):
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    fp = FaceProcessor(output_size=112, detector=det, quality_filter_config={"min_det_score": 0.0, "min_face_size": 0})
    imgs = [_noise(300 + i, H, W) for i, (H, W) in enumerate([(540, 960), (481, 367), (240, 240), (360, 500),
                                                              (600, 1400)])]
    got = fp.process_images(imgs, return_all=True)
    want = [fp.process_numpy(im, return_all=True) for im in imgs]
    assert sum(len(w) for w in want) > 5
    for g, w in zip(got, want):
        _match_faces(g, w)
        assert all(r["aligned_face"].shape == (112, 112, 3) for r in g)


# 9 ------------------------------------------------------------------------------------------------
def test_dataset_preprocessor_end_to_end(det, tmp_path):
    from PIL import Image
    from facerecognitionpipeline_amd.dataset_preprocessor import DEFAULT_QUALITY_CONFIG, DatasetPreprocessor
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    tree = tmp_path / "classroom"
    files = [("s01/center/a.png", (240, 320)), ("s01/center/b.png", (300, 200)), ("s01/left/c.png", (180, 180)),
             ("s02/img_right.png", (300, 200)), ("s02/plain.png", (240, 320)), ("s02/x_left.png", (180, 180)),
             ("s02/broken.jpg", None)]
    for i, (rel, size) in enumerate(files):
        os.makedirs(tree / os.path.dirname(rel), exist_ok=True)
        if size is None:
            (tree / rel).write_bytes(b"not an image")
        else:
            Image.fromarray(_noise(500 + i, *size)).save(tree / rel)
    fp = FaceProcessor(output_size=224, detector=det, quality_filter_config=dict(DEFAULT_QUALITY_CONFIG))
    out = tmp_path / "out"
    DatasetPreprocessor(processor=fp, batch_size=4, verbose=False).process_dataset(str(tree), str(out))
    with open(out / "probe_positive_metadata.json") as f:
        meta = json.load(f)
    walk = [("s01/center/a.png", "s01", "center", 1), ("s01/center/b.png", "s01", "center", 2),
            ("s01/left/c.png", "s01", "left", 1), ("s02/broken.jpg", "s02", "center", 1),
            ("s02/img_right.png", "s02", "right", 2), ("s02/plain.png", "s02", "center", 3),
            ("s02/x_left.png", "s02", "left", 4)]
    at = 0
    for rel, cls, angle, idx in walk:
        want = [] if rel.endswith("broken.jpg") else fp.process_image(str(tree / rel), return_all=True)
        mine = meta[at:at + len(want)]
        at += len(want)
        std = f"{cls}_{angle}_{idx:03d}"
        for k, m in enumerate(mine):
            assert (m["filename"], m["class_id"], m["source_image"], m["standardized_name"], m["face_index"],
                    m["angle"]) == (f"{std}_face{k}.jpg", cls, os.path.basename(rel), f"{std}.jpg", k, angle)
            assert type(m["det_score"]) is float and type(m["face_size"]) is int and type(m["bbox"]) is list
            with Image.open(out / "probe_positive" / m["filename"]) as im:
                assert im.size == (224, 224)
        _match_faces([{"bbox": np.array(m["bbox"]), "det_score": m["det_score"]} for m in mine], want)
    assert at == len(meta) > 0
    assert len(os.listdir(out / "probe_positive")) == len(meta)
