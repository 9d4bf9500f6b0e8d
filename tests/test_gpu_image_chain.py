"""The mixed-size device chain: ``fr_detect_images_device`` / ``fr_align_images_device`` (photographs of
different sizes to detections, crops and gate outputs in HBM, nothing staged and nothing waited for)
and what stands on them -- ``Handle.detect_images_device`` / ``align_images_device``, the torch ops,
``device_chain_images``, ``FaceProcessor.process_images(gate="device")`` and
``FaceMatcher.match_images(device_chain=True)``.

Everything is compared bitwise with the host route of tests/test_gpu_image_batches.py (the same
images, the same chunks of MAX_FRAMES = 4: 4, 4 and 1 with portrait, 1 x 1 and 2 x 3 images), but yaw
and roll, which follow the rule of tests/test_gpu_quality_gate.py.  F = 8 slots per image: the
synthetic detector finds tens of faces in each noise image (55 to 81 at 0.5, and 12 in the 2 x 3 one),
so their slots are all live unless counts are planted; the 1 x 1 image gives 5, so three of its slots
are not.  (The premise that every noise image gives about 60 faces, and so more than F, does not hold
for that one image: ``_assert_counts`` asserts "more than F" for the other eight and 2 <= count < F for
it.)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _fit_sets, _frt
from tests import _gate_device_inputs as gi
from tests.test_gpu_detector_rows import _frames
from tests.test_gpu_image_batches import MAX_FRAMES, SIZES

pytestmark = pytest.mark.gpu

F = 8
THRESH = 0.5
TINY = SIZES.index((1, 1))  # the one image with fewer faces than slots
# the limits of tests/test_gpu_quality_gate.py's process_frames test, for the same detector on noise
GATE_CONFIG = {"min_det_score": 0.61, "min_face_size": 10, "max_yaw": 100, "max_pitch": 1e9, "max_roll": 40,
               "blur_threshold": 2.0}


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def det():
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_recognition import FaceDetector
    return FaceDetector(state_dict=synthetic_detector_state_dict(), max_frames=MAX_FRAMES, max_faces=F,
                        det_thresh=THRESH)


@pytest.fixture(scope="module")
def ops():
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", torch.cuda.current_device()), max_batch=1)


def _noise_images(seed0):
    return [_frames(seed0 + sum(s) + i, 1, *s)[0].contiguous() for i, s in enumerate(SIZES)]


@pytest.fixture(scope="module")
def images():
    return _noise_images(0)


@pytest.fixture(scope="module")
def host_dets(det, images):
    """detect_images' (dets, counts) at F rows: the reference of the detect, align and op tests."""
    dets, counts = det.model.detect_images(images, THRESH, F)
    print("detect_images counts", counts.tolist())
    _assert_counts(counts)
    return dets, counts


def _assert_counts(counts):
    """What the tests rely on: every image but the 1 x 1 one has more faces than slots, that one at
    least two."""
    counts = np.asarray(counts)
    assert (np.delete(counts, TINY) > F).all() and 2 <= counts[TINY] < F, counts.tolist()


def _assert_rows_equal(dev, host, max_faces):
    (d_dets, d_counts), (h_dets, h_counts) = dev, host
    assert d_dets.shape == h_dets.shape and d_counts.dtype == torch.int32
    assert np.array_equal(d_counts.cpu().numpy(), h_counts)
    d = d_dets.cpu().numpy()
    for f, c in enumerate(h_counts):
        k = min(int(c), max_faces)
        assert np.array_equal(d[f, :k].view(np.uint32), h_dets[f, :k].view(np.uint32)), f


# 1 ------------------------------------------------------------------------------------------------
def _table_lib():
    L = _frt.lib()
    for fn in (L.frt_resize_axis_table, L.frt_resize_tables_device):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return L


@pytest.mark.parametrize("dsize,ssize", [(640, 1920), (360, 1080), (640, 640), (640, 1), (1, 1), (426, 2), (640, 3),
                                         (53, 37), (640, 8192), (1, 8192), (7, 5), (112, 224)])
def test_device_tables_are_the_host_tables(dsize, ssize):
    """Up-scaling, down-scaling, identity, both clamps, the largest side and the 112-wide crop case."""
    from facerecognitionpipeline_amd import _lib
    L = _table_lib()
    want = np.full((dsize, 4), -7, np.int32)
    got = np.full((dsize, 4), -9, np.int32)
    _lib.check(L.frt_resize_axis_table(dsize, ssize, want.ctypes.data))
    _lib.check(L.frt_resize_tables_device(dsize, ssize, got.ctypes.data))
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    assert (want[:, 2] + want[:, 3] == 2048).all() and want[:, :2].min() >= 0 and want[:, :2].max() <= ssize - 1


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_reduction", [1, 0])
def test_detect_images_device_is_detect_images(det, images, row_reduction):
    m = det.model
    frames = _frames(2000, 3, 720, 1280)
    try:
        _frt.set_detector_row_reduction(m, row_reduction)
        for max_faces in (1024, F):
            want = m.detect_images(images, THRESH, max_faces)
            _assert_counts(want[1])
            _assert_rows_equal(m.detect_images_device(images, THRESH, max_faces), want, max_faces)
        # images of one size: detect_device's launches on detect_device's canvases
        d_img, c_img = m.detect_images_device([frames[i] for i in range(3)], THRESH, 256)
        d_ref, c_ref = m.detect_device(frames, THRESH, 256)
    finally:
        _frt.set_detector_row_reduction(m, 1)
    assert c_ref.min() > 0 and torch.equal(c_img, c_ref)
    assert torch.equal(d_img.view(torch.int32), d_ref.view(torch.int32))


# 3 ------------------------------------------------------------------------------------------------
def test_candidate_limit_marks_the_image(det, images, host_dets):
    with pytest.raises(NotImplementedError):
        det.model.detect_images(images, 0.0, F)
    _, counts = det.model.detect_images_device(images, 0.0, F)
    assert counts.cpu().tolist() == [-1] * len(images)
    _assert_rows_equal(det.model.detect_images_device(images, THRESH, F), host_dets, F)  # and works on


# 4 ------------------------------------------------------------------------------------------------
def _host_align(ops, images, lm, S):
    """fr_align_images of the faces lm[i][k] the host fit accepts -> (ok [n,F], crops [n,F,S,S,3],
    tforms [n,F,2,3]) with zeros / NaN where it refuses."""
    from tests.test_gpu_device_chain import _fit_lib
    L, t = _fit_lib(), _fit_sets.template(S)
    n, Fs = lm.shape[:2]
    ok = np.zeros((n, Fs), np.uint8)
    M = np.empty(6)
    for i in range(n):
        for k in range(Fs):
            ok[i, k] = L.frt_fit_similarity(np.ascontiguousarray(lm[i, k]).ctypes.data, t.ctypes.data, 5,
                                            M.ctypes.data) == 0
    at = np.argwhere(ok == 1)
    out = torch.empty((len(at), S, S, 3), dtype=torch.uint8, device="cuda")
    tf = ops.align_images(images, np.ascontiguousarray(lm[ok == 1]), at[:, 0].astype(np.int32), S, out)
    crops = np.zeros((n, Fs, S, S, 3), np.uint8)
    tforms = np.full((n, Fs, 2, 3), np.nan)
    crops[ok == 1], tforms[ok == 1] = out.cpu().numpy(), tf
    return ok, crops, tforms


def _assert_aligned(got, want, live=None):
    crops, tforms, ok = (x.cpu().numpy() for x in got)
    w_ok, w_crops, w_tf = want
    if live is not None:
        w_ok = w_ok * live
    assert np.array_equal(ok, w_ok)
    on = w_ok == 1
    assert np.array_equal(crops[on], w_crops[on])
    same = (_bits(tforms[on]) == _bits(w_tf[on])).reshape(int(on.sum()), -1).all(axis=1)
    assert same.all(), np.argwhere(on)[~same][:8]
    assert not crops[~on].any() and np.isnan(tforms[~on]).all()
    return int(on.sum())


@pytest.mark.parametrize("S", [112, 224])
def test_align_images_device_is_align_images_per_slot(ops, images, host_dets, S):
    """The detect rows in place (stride 15) with the detector's counts, then counts planted over the
    same rows (-1, 0, 3 and beyond F in turn): slots past the count hold real detections and must
    still come back empty."""
    dets, counts = host_dets
    n = len(images)
    full = (np.arange(F)[None] < counts[:, None]).astype(np.uint8)
    lm = dets[:, :, 5:].reshape(n, F, 5, 2).copy()
    lm[full == 0] = 0  # rows past the count are not detect_images' to define: a set the host fit refuses
    want = _host_align(ops, images, lm, S)
    assert np.array_equal(want[0], full)  # the synthetic detector's landmark sets all fit on the host
    d_dets = torch.from_numpy(dets).cuda()
    got = ops.align_images_device(images, d_dets, torch.from_numpy(counts).cuda(), S)
    assert _assert_aligned(got, want) == int(full.sum()) == n * F - (F - counts[TINY])
    assert (got[0].cpu().numpy().reshape(n * F, -1) != 0).any(axis=1).sum() > n * F // 2  # most crops have content
    planted = np.array([(-1, 0, 3, F + 5)[i % 4] for i in range(n)], np.int32)
    live = (np.arange(F)[None] < planted[:, None]).astype(np.uint8) * full
    d_dets[torch.from_numpy(full == 0).cuda()] = 1e4  # past the detector's count: never live, whatever is there
    got = ops.align_images_device(images, d_dets, torch.from_numpy(np.minimum(planted, counts)).cuda(), S)
    assert _assert_aligned(got, want, live) == int(live.sum()) and 0 < live.sum() < n * F


def test_align_images_device_splits_long_lists_and_refuses_fits(ops):
    """One more image than a fit launch takes by value, so the list splits into two launches; planted
    landmarks [n,F,5,2] with counts=None.  Tiny images (8 x 8 up to 16 x 24, sizes cycling); odd slots
    get their landmark set shrunk into the image, so that the crop shows that image and no other."""
    S = 112
    L = _frt.lib()
    L.frt_fit_images_by_value.restype = ctypes.c_int
    L.frt_fit_images_by_value.argtypes = []
    FIT_IMAGES_BY_VALUE = L.frt_fit_images_by_value()  # frhip_kernels.h: images per fit launch
    assert 1 <= FIT_IMAGES_BY_VALUE <= 240  # 16 bytes each beside FitSlots, under the 4 KB argument limit
    n = FIT_IMAGES_BY_VALUE + 1
    r = np.random.default_rng(4)
    sizes = [(8, 8), (9, 16), (16, 11), (13, 13), (16, 24)]
    imgs = [torch.from_numpy(r.integers(0, 256, (*sizes[i % 5], 3), dtype=np.uint8)).cuda() for i in range(n)]
    sets = _fit_sets.landmark_sets(S)
    lm = np.empty((n, F, 5, 2), np.float32)
    for i in range(n):
        H, W = sizes[i % 5]
        for k in range(F):
            base = sets[(i * F + k) % len(sets)].astype(np.float64)
            if k % 2:
                dev = base - base.mean(0)
                spread = np.abs(dev).max()
                base = dev * (min(H, W) / 4 / spread if spread else 0.0) + (W / 2, H / 2)
            lm[i, k] = base.astype(np.float32)
    want = _host_align(ops, imgs, lm, S)
    assert 0 < (want[0] == 0).sum() < 64 and (want[0][FIT_IMAGES_BY_VALUE:] == 1).any()  # both outcomes, both launches
    got = ops.align_images_device(imgs, torch.from_numpy(lm).cuda(), None, S)
    _assert_aligned(got, want)
    filled = (got[0].cpu().numpy().reshape(n, F, -1) != 0).any(axis=2)
    assert filled[:, 1::2][want[0][:, 1::2] == 1].all() and filled[-1].any()


# 5 ------------------------------------------------------------------------------------------------
def _chain(det, ops, imgs, cfg, bufs=None):
    b = bufs or {}
    dets, counts = det.model.detect_images_device(imgs, THRESH, F, b.get("dets"), b.get("counts"))
    crops, tforms, ok = ops.align_images_device(imgs, dets, counts, 112, b.get("crops"), b.get("tforms"), b.get("ok"))
    blur = ops.blur_scores_device(crops.view(-1, 112, 112, 3), b.get("blur"))
    gate = ops.quality_gate_device(dets, counts, ok, blur, cfg, b.get("gate"))
    return {"dets": dets, "counts": counts, "crops": crops, "tforms": tforms, "ok": ok, "blur": blur, "gate": gate}


def test_chain_is_capturable_in_a_graph(det, ops):
    """No synchronisation, no allocation, no pageable copy: after one eager warm-up the four calls are
    captured on fixed buffers and replay on new image contents to the eager results, bit for bit.
    Five images of five sizes: a chunk of four and a chunk of one.

    A chunk is kernel launches only (the table kernel zeroes the chunk's candidate counters), which
    is what this pins: a counter that is not zero on replay shows as counts of -1."""
    from facerecognitionpipeline_amd.face_recognition import _gate_config, quality_gate_host
    cfg = _gate_config(GATE_CONFIG)
    sizes = SIZES[1:6]
    bufs_img = [_frames(10 + i, 1, *s)[0].contiguous() for i, s in enumerate(sizes)]
    bufs = _chain(det, ops, bufs_img, cfg)  # warm-up: the slot buffer, the gate's and the convs' workspaces
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _chain(det, ops, bufs_img, cfg, bufs)
    for seed in (78, 79):
        new = [_frames(seed + i, 1, *s)[0].contiguous() for i, s in enumerate(sizes)]
        want = _chain(det, ops, new, cfg)
        want = {k: ({q: t.clone() for q, t in v.items()} if k == "gate" else v.clone()) for k, v in want.items()}
        for b, x in zip(bufs_img, new):
            b.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        counts = want["counts"].cpu().numpy()
        assert np.array_equal(bufs["counts"].cpu().numpy(), counts) and counts.min() > 0
        for f, c in enumerate(counts):  # rows past the count are not written
            assert torch.equal(bufs["dets"][f, :min(c, F)].view(torch.int32),
                               want["dets"][f, :min(c, F)].view(torch.int32))
        assert torch.equal(bufs["ok"], want["ok"]) and torch.equal(bufs["crops"], want["crops"])
        assert np.array_equal(_bits(bufs["tforms"]), _bits(want["tforms"]))
        assert np.array_equal(_bits(bufs["blur"]), _bits(want["blur"]))
        for k in gi.OUTPUTS:
            assert torch.equal(bufs["gate"][k].view(torch.uint8), want["gate"][k].view(torch.uint8)), k
        assert int(bufs["gate"]["frame_offsets"][-1]) >= 2
        # and the gate of the chain is the host statement on the chain's own outputs
        host = quality_gate_host(bufs["dets"].cpu().numpy(), counts, bufs["ok"].cpu().numpy(),
                                 bufs["blur"].cpu().numpy().reshape(len(sizes), F), cfg)
        gi.assert_same_gate({k: v.cpu().numpy() for k, v in bufs["gate"].items()}, dict(zip(gi.OUTPUTS, host)), seed)


# 6 ------------------------------------------------------------------------------------------------
def test_arguments(det, ops):
    from facerecognitionpipeline_amd import _lib
    m = det.model
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    good = torch.zeros((40, 50, 3), dtype=torch.uint8, device="cuda")
    empty = torch.zeros((0, 50, 3), dtype=torch.uint8, device="cuda")
    dets = torch.full((3, F, 15), 7.0, device="cuda")
    counts = torch.full((3,), 7, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((dets == 7).all()) and bool((counts == 7).all())

    with pytest.raises(ValueError, match="image 2"):                             # a NULL pointer
        m.detect_images_device([good, good, empty], THRESH, F, dets, counts)
    with pytest.raises(ValueError, match="image 1 .*8193"):                      # a side above 8192
        m.detect_images_device([good, torch.zeros((8193, 1, 3), dtype=torch.uint8, device="cuda"), good], THRESH, F,
                               dets, counts)
    with pytest.raises(ValueError, match="image 1 is too small to letterbox"):
        m.detect_images_device([good, torch.zeros((1, 700, 3), dtype=torch.uint8, device="cuda"), good], THRESH, F,
                               dets, counts)
    with pytest.raises(ValueError, match="max_faces"):
        m.detect_images_device([good], THRESH, 0)
    # a side of 0 behind a pointer that is not NULL: the C call itself
    ptrs = np.array([good.data_ptr()] * 3, np.uint64)
    sizes = np.array([[40, 50], [0, 50], [40, 50]], np.int32)
    rc = L.fr_detect_images_device(m.h, ptrs.ctypes.data, sizes.ctypes.data, 3, THRESH, F, dets.data_ptr(),
                                   counts.data_ptr(), stream)
    assert rc == _lib.FR_ERR_INVALID_ARGUMENT and b"image 1" in L.fr_last_error(m.h)
    assert untouched()
    for bad in (good.float(), good[:, :, :2], good[0], good.cpu()):
        with pytest.raises(ValueError):
            m.detect_images_device([bad], THRESH, F)
    d, c = m.detect_images_device([], THRESH, F)                                 # n == 0: a no-op
    assert d.shape == (0, F, 15) and c.shape == (0,)
    with pytest.raises(_lib.FrHipError):                                         # not a detector handle
        ops.detect_images_device([good], THRESH, F)

    # fr_align_images_device (any handle)
    lm = torch.zeros((3, F, 15), device="cuda")
    crops = torch.full((3, F, 112, 112, 3), 7, dtype=torch.uint8, device="cuda")
    ok = torch.full((3, F), 7, dtype=torch.uint8, device="cuda")
    three = [good, good, good]
    with pytest.raises(ValueError, match="image 2"):                             # a NULL pointer
        ops.align_images_device([good, good, empty], lm, None, 112, crops, None, ok)
    for S in (0, 1025):
        with pytest.raises(ValueError):
            ops.align_images_device([good], lm[:1, :1], None, S)
    sizes[1] = [40, 50]
    for stride, size1, out_size in ((9, 40, 112), (15, 0, 112), (15, 40, 0), (15, 40, 1025)):
        sizes[1, 0] = size1
        rc = L.fr_align_images_device(ops.h, ptrs.ctypes.data, sizes.ctypes.data, 3, lm.data_ptr(), stride, None, F,
                                      out_size, crops.data_ptr(), None, ok.data_ptr(), stream)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, (stride, size1, out_size)
    torch.cuda.synchronize()
    assert bool((crops == 7).all()) and bool((ok == 7).all())
    for bad_lm in (lm[:2], lm[:, :, :14], lm.double(), lm.cpu()):
        with pytest.raises(ValueError):
            ops.align_images_device(three, bad_lm, None, 112)
    with pytest.raises(ValueError):                                              # counts of another length
        ops.align_images_device(three, lm, torch.zeros(2, dtype=torch.int32, device="cuda"), 112)
    with pytest.raises(ValueError):                                              # an image on the host
        ops.align_images_device([good.cpu()] * 3, lm, None, 112)
    out, tf, k = ops.align_images_device([], lm[:0], None, 112)                  # no image: a no-op
    assert out.shape == (0, F, 112, 112, 3) and tf.shape == (0, F, 2, 3) and k.shape == (0, F)
    # an image without a live slot may be anything valid: no pixel of it is read
    out, _, k = ops.align_images_device([good[:1, :1]] * 3, lm, torch.zeros(3, dtype=torch.int32, device="cuda"), 112)
    assert not out.any() and not k.any()


# 6b -----------------------------------------------------------------------------------------------
def test_device_chain_images_over_three_blocks(det, images, host_dets):
    """``device_chain_images`` without ``pick`` over the nine images (blocks of 4, 4 and 1): the merged
    host and device outputs are those of the blocks with slot numbers counted over all images, the
    crops are every slot's, and ``chain_faces`` lists each image as the chain of that image's own block
    does."""
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor, chain_faces, device_chain_images
    fp = FaceProcessor(output_size=112, detector=det, quality_filter_config=dict(GATE_CONFIG))
    args = (det, fp.aligner, fp.quality_filter)
    n = len(images)
    host, gate, crops = device_chain_images(*args, images)
    live = np.minimum(host_dets[1], F)
    assert tuple(crops.shape) == (n * F, 112, 112, 3) and host["stage"].shape == (n, F)
    assert np.array_equal(host["counts"], host_dets[1])
    assert host["frame_offsets"].tolist() == [0] + np.cumsum(live).tolist()
    total, n_valid = int(live.sum()), int(host["n_valid"][0])
    assert sorted(host["rows"][:total].tolist()) == [i * F + k for i in range(n) for k in range(live[i])]
    assert (host["rows"][total:] == -1).all() and (host["valid_slots"][n_valid:] == -1).all()
    assert n_valid == int((host["stage"] == 0).sum()) and host["rows"].shape == host["valid_slots"].shape == (n * F,)
    for k, t in gate.items():  # the merged device tensors are the merged host arrays
        assert t.dtype == torch.from_numpy(host[k]).dtype and np.array_equal(t.cpu().numpy(), host[k]), k
    all_crops = crops.cpu().numpy()
    assert (all_crops.reshape(n * F, -1) != 0).any(axis=1).sum() > n * F // 2  # most crops have content
    for first in range(0, n, MAX_FRAMES):
        block = images[first:first + MAX_FRAMES]
        h_b, _g, c_b = device_chain_images(*args, block)  # one block: the unmerged return
        c_b = c_b.cpu().numpy()
        for j in range(len(block)):
            got, want = chain_faces(fp.quality_filter, host, first + j), chain_faces(fp.quality_filter, h_b, j)
            assert len(got) == len(want) == live[first + j]
            for a, b in zip(got, want):
                assert a["slot"] == b["slot"] + first * F and a["is_valid"] == b["is_valid"]
                assert np.array_equal(a["bbox"], b["bbox"]) and np.array_equal(a["landmarks"], b["landmarks"])
                assert a["quality_metrics"] == b["quality_metrics"]
                assert np.array_equal(all_crops[a["slot"]], c_b[b["slot"]])
    # pick: only what it returns is kept, block after block
    host_p, _g, kept = device_chain_images(
        *args, images, pick=lambda h, g, c: c[g["rows"][:int(h["frame_offsets"][-1])].long()])
    assert np.array_equal(host_p["rows"], host["rows"])
    assert np.array_equal(kept.cpu().numpy(), all_crops[host["rows"][:total]])


# 7 ------------------------------------------------------------------------------------------------
def _same_face(g, w):
    from tests.test_gpu_quality_gate import _same_metrics
    assert list(g) == list(w)
    assert g["det_score"] == w["det_score"] and g["is_valid"] == w["is_valid"]
    assert g["bbox"].dtype == w["bbox"].dtype and np.array_equal(g["bbox"], w["bbox"])
    assert g["landmarks"].dtype == w["landmarks"].dtype and np.array_equal(g["landmarks"], w["landmarks"])
    assert g["aligned_face"].shape == w["aligned_face"].shape and np.array_equal(g["aligned_face"], w["aligned_face"])
    _same_metrics(g["quality_metrics"], w["quality_metrics"])


def _photographs(images):
    """The nine images on the host plus a gray one."""
    photos = [im.cpu().numpy() for im in images]
    return photos + [np.ascontiguousarray(photos[1][:, :, 1])]


@pytest.mark.parametrize("return_all", [False, True])
def test_process_images_device_gate_is_the_host_gate(det, images, host_dets, return_all, tmp_path):
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    fp = FaceProcessor(output_size=112, detector=det, quality_filter_config=dict(GATE_CONFIG))
    photos = _photographs(images)
    want = fp.process_images(photos, return_all=return_all)
    got = fp.process_images(photos, return_all=return_all, gate="device")
    assert len(got) == len(want) == len(photos)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            _same_face(a, b)
    flags = [r["is_valid"] for fs in got for r in fs]
    print("faces per image", [len(fs) for fs in got], "valid", sum(flags))
    if return_all:
        assert [len(fs) for fs in got[:-1]] == np.minimum(host_dets[1], F).tolist() and len(got[-1]) >= 2
        assert got[-1][0]["aligned_face"].ndim == 2
        assert any(r["aligned_face"].any() for fs in got for r in fs)
    else:
        assert all(flags) and max(len(fs) for fs in got) <= 1
    # one undecodable path keeps its slot
    bad = str(tmp_path / "bad.png")
    with open(bad, "wb") as f:
        f.write(b"no image")
    with pytest.raises(ValueError, match="Could not load image"):
        fp.process_images([photos[2], bad], return_all, gate="device")
    out = fp.process_images([photos[2], bad, photos[9]], return_all, errors="return", gate="device")
    assert isinstance(out[1], ValueError)
    ref = fp.process_images([photos[2], photos[9]], return_all)
    for g, w in zip((out[0], out[2]), ref):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            _same_face(a, b)
    assert fp.process_images([], return_all, gate="device") == []
    det.det_thresh = 0.0
    try:
        with pytest.raises(NotImplementedError, match="image 0"):
            fp.process_images(photos[1:3], gate="device")
    finally:
        det.det_thresh = THRESH


# 8 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def embedder():
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    return FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=64)


@pytest.mark.parametrize("exclusive", [False, True])
def test_match_images_device_chain_is_match_images(det, embedder, images, exclusive, tmp_path):
    """The embedder, gallery and processor of tests/test_gpu_match_images.py."""
    from facerecognitionpipeline_amd import weights as W
    from tests.test_gpu_match_images import _matcher, _processor
    from tests.test_gpu_quality_gate import _same_metrics
    emb = embedder
    fp = _processor(det)
    photos = _photographs(images)[1:]  # eight images of different sizes and the gray one
    faces = [fs for fs in fp.process_images(photos, return_all=True) if fs]
    enrolled = [faces[0][0], faces[0][-1], faces[1][0]]
    students = [(f"S{i:03d}", f"Student {i}", r["aligned_face"]) for i, r in enumerate(enrolled)]
    students += [(f"U{i:03d}", f"Unrelated {i}", c) for i, c in enumerate(W.synthetic_crops(5))]
    fm = _matcher(emb, tmp_path / "students.npz", students, fp)
    want = fm.match_images(photos, top_k=3, exclusive=exclusive)
    got = fm.match_images(photos, top_k=3, exclusive=exclusive, device_chain=True)
    assert len(got) == len(want) == len(photos)
    for g, w in zip(got, want):
        assert list(g) == list(w) and isinstance(g["timestamp"], str)
        for k in w:
            if k not in ("timestamp", "matches"):
                assert g[k] == w[k], k
        assert len(g["matches"]) == len(w["matches"]) >= 2
        for a, b in zip(g["matches"], w["matches"]):
            assert list(a) == list(b)
            for k in b:
                if k == "quality_metrics":
                    _same_metrics(a[k], b[k])
                else:
                    assert a[k] == b[k], k
    assert sum(g["num_recognized"] for g in got) >= 3
    assert any(not m["recognized"] for g in got for m in g["matches"])
    assert fm.match_images([], device_chain=True) == []


# 9 ------------------------------------------------------------------------------------------------
def test_torch_ops_are_the_handle_methods(det, ops, images):
    from facerecognitionpipeline_amd import torch_ops
    imgs = images[1:6]
    hid = torch_ops.register(det.model)
    try:
        want_d, want_c = det.model.detect_images_device(imgs, THRESH, F)
        want = ops.align_images_device(imgs, want_d, want_c, 112)
        dets, counts = torch.ops.frhip.detect_images(imgs, hid, THRESH, F)
        crops, tforms, ok = torch.ops.frhip.align_image_detections(imgs, dets, counts, 112)
        with pytest.raises(ValueError):  # CPU tensors: there is no CPU fallback
            torch.ops.frhip.detect_images([im.cpu() for im in imgs], hid, THRESH, F)
        with pytest.raises(ValueError):
            torch.ops.frhip.align_image_detections([im.cpu() for im in imgs], dets, counts, 112)
    finally:
        torch_ops.unregister(hid)
    assert torch.equal(counts, want_c) and torch.equal(dets.view(torch.int32), want_d.view(torch.int32))
    assert torch.equal(crops, want[0]) and torch.equal(ok, want[2]) and bool(ok.all())
    assert np.array_equal(_bits(tforms), _bits(want[1]))
