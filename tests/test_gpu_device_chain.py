"""The device-resident detect -> align -> blur chain (fr_detect_device, fr_align_device,
fr_blur_scores_device) against the host-output calls it restates, bit for bit:

1. the fit kernel against the host fit (frt_fit_similarity) on planted landmark sets,
2. detect_device against detect, 3. align_device against align_faces per face,
4. blur_scores_device against blur_scores, 5. the three captured in one graph (a synchronisation,
an allocation or a pageable copy in any of them fails the capture), 6. the torch ops against the
Handle methods, 7. RecognitionPipeline.recognize_frames against recognize per frame.

Small shapes: 3 noise frames of 135 x 240 with max_frames = 2 (a chunk of 2 and a tail of 1); the
detector's cost is its 640 x 640 canvas either way.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _fit_sets

pytestmark = pytest.mark.gpu

H, W, N_FRAMES, MAX_FACES = 135, 240, 3, 8
THRESH = 0.5


def _bits(a):
    """float64 array (or tensor) -> its uint64 bit patterns (NaNs compare by payload)."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _noise_frames(seed, n=N_FRAMES):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda()


@pytest.fixture(scope="module")
def det():
    from facerecognitionpipeline_amd.detector_arch import synthetic_detector_state_dict
    from facerecognitionpipeline_amd.face_recognition import FaceDetector
    return FaceDetector(state_dict=synthetic_detector_state_dict(), max_frames=2, max_faces=MAX_FACES,
                        det_thresh=THRESH)


@pytest.fixture(scope="module")
def ops():
    """A model-less handle for align / blur."""
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", torch.cuda.current_device()), max_batch=1)


@pytest.fixture(scope="module")
def frames():
    return _noise_frames(77)


@pytest.fixture(scope="module")
def host_dets(det, frames):
    """detect's (dets, counts) of the frames: the reference of tests 2 and 3, computed once."""
    dets, counts = det.model.detect(frames, THRESH, MAX_FACES)
    print("detect counts", counts.tolist())
    assert counts.max() >= 2, "the frames must give some frame two faces or more"
    return dets, counts


@pytest.fixture(scope="module")
def dev_dets(det, frames):
    dets, counts = det.model.detect_device(frames, THRESH, MAX_FACES)
    torch.cuda.synchronize()
    return dets, counts


# 1 ------------------------------------------------------------------------------------------------
def _fit_lib():
    from facerecognitionpipeline_amd import _lib
    L = _lib.load()
    L.frt_fit_similarity.restype = ctypes.c_int
    L.frt_fit_similarity.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p]
    L.frt_fit_similarity_device.restype = ctypes.c_int
    L.frt_fit_similarity_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    return L


@functools.lru_cache(maxsize=None)
def _host_fits(S):
    """(sets, host maps [n,6] with NaN rows where the host fit fails, host ok [n]) for out_size S."""
    L = _fit_lib()
    sets, t = _fit_sets.landmark_sets(S), _fit_sets.template(S)
    M = np.full((len(sets), 6), np.nan)
    ok = np.zeros(len(sets), dtype=np.uint8)
    for i, lm in enumerate(sets):
        ok[i] = L.frt_fit_similarity(lm.ctypes.data, t.ctypes.data, 5, M[i].ctypes.data) == 0
    assert ok[0] and not ok[1] and not ok[64] and ok.sum() >= len(sets) - 4  # both outcomes, as planted
    return sets, M, ok


@pytest.mark.parametrize("n", [1, 63, 65, 130])
@pytest.mark.parametrize("S", [112, 224])
def test_fit_kernel_is_the_host_fit(S, n):
    from facerecognitionpipeline_amd import _lib
    sets, want, want_ok = _host_fits(S)
    lm = np.ascontiguousarray(sets[:n])
    M = np.zeros((n, 6))
    ok = np.full(n, 7, dtype=np.uint8)
    _lib.check(_fit_lib().frt_fit_similarity_device(lm.ctypes.data, n, S, M.ctypes.data, ok.ctypes.data, None))
    assert np.array_equal(ok, want_ok[:n])
    assert np.isnan(M[ok == 0]).all()
    same = (_bits(M[ok == 1]) == _bits(want[:n][ok == 1])).all(axis=1)
    assert same.all(), np.flatnonzero(ok == 1)[~same]


# 2 ------------------------------------------------------------------------------------------------
def _assert_rows_equal(dev, host, max_faces):
    (d_dets, d_counts), (h_dets, h_counts) = dev, host
    assert np.array_equal(d_counts.cpu().numpy(), h_counts)
    d = d_dets.cpu().numpy()
    for f, c in enumerate(h_counts):
        k = min(int(c), max_faces)
        assert np.array_equal(d[f, :k].view(np.uint32), h_dets[f, :k].view(np.uint32)), f


def test_detect_device_is_detect(det, frames, host_dets, dev_dets):
    assert dev_dets[0].shape == (N_FRAMES, MAX_FACES, 15) and dev_dets[1].dtype == torch.int32
    _assert_rows_equal(dev_dets, host_dets, MAX_FACES)
    small = int(host_dets[1].max()) - 1  # fewer rows than the fullest frame has faces
    assert small >= 1
    host_small = det.model.detect(frames, THRESH, small)
    assert np.array_equal(host_small[1], host_dets[1])  # counts are the full kept counts
    _assert_rows_equal(det.model.detect_device(frames, THRESH, small), host_small, small)


def test_detect_device_marks_frames_over_the_candidate_limit(det, frames, host_dets):
    with pytest.raises(NotImplementedError):
        det.model.detect(frames, 0.0, MAX_FACES)
    _, counts = det.model.detect_device(frames, 0.0, MAX_FACES)
    assert counts.cpu().tolist() == [-1] * N_FRAMES
    _assert_rows_equal(det.model.detect_device(frames, THRESH, MAX_FACES), host_dets, MAX_FACES)  # and works on


# 3 ------------------------------------------------------------------------------------------------
def _align_one(ops, frame, lm, S):
    out = torch.empty((1, S, S, 3), dtype=torch.uint8, device=frame.device)
    tf = ops.align_faces(frame, lm[None], S, out)
    return out[0].cpu().numpy(), tf[0]


_WANT = {}  # (frame, face, out_size) -> align_faces of that face alone: shared by the cases below


def _want_slot(ops, frames, host_dets, f, i, S):
    if (f, i, S) not in _WANT:
        _WANT[f, i, S] = _align_one(ops, frames[f], host_dets[0][f, i, 5:].reshape(5, 2), S)
    return _WANT[f, i, S]


@pytest.mark.parametrize("case", ["detected", "planted"])
@pytest.mark.parametrize("S", [112, 224])
def test_align_device_is_align_faces_per_slot(ops, frames, host_dets, dev_dets, S, case):
    """Every live slot is align_faces of that face alone; every other slot is ok = 0 and zeros.
    "detected": the detector's own counts (the noise frames give every frame more faces than
    MAX_FACES, so all slots are live).  "planted": counts -1 (detect_device's overflow mark), 0 and 3
    over the same rows: slots past the count hold real detections and must still come back empty."""
    dets, counts = dev_dets
    full = np.minimum(host_dets[1], MAX_FACES)
    live = full if case == "detected" else np.array([-1, 0, min(3, int(full[2]))])
    if case == "planted":
        counts = torch.from_numpy(live.astype(np.int32)).cuda()
    crops, tforms, ok = ops.align_device(frames, dets, counts, S)
    crops, tforms, ok = crops.cpu().numpy(), tforms.cpu().numpy(), ok.cpu().numpy()
    n_ok = 0
    for f in range(N_FRAMES):
        for i in range(MAX_FACES):
            if i < live[f]:  # the synthetic detector's landmark sets all fit on the host
                want, want_tf = _want_slot(ops, frames, host_dets, f, i, S)
                assert ok[f, i] == 1
                assert np.array_equal(crops[f, i], want), (f, i)
                assert np.array_equal(_bits(tforms[f, i]), _bits(want_tf)), (f, i)
                n_ok += 1
            else:
                assert ok[f, i] == 0 and not crops[f, i].any() and np.isnan(tforms[f, i]).all(), (f, i)
    assert n_ok >= 2 and (case == "detected" or n_ok < N_FRAMES * MAX_FACES)


@pytest.mark.parametrize("S", [112, 224])
def test_align_device_plain_form_and_refused_fits(ops, frames, S):
    """One frame, landmarks [1,F,5,2] (stride 10), no counts: every slot is live; the sets the host
    fit refuses come back ok = 0 with all-zero crops."""
    sets, _, host_ok = _host_fits(S)
    lm, host_ok = sets[:12].copy(), host_ok[:12]  # set 0, the template itself, lies inside the frame
    crops, tforms, ok = ops.align_device(frames[:1], torch.from_numpy(lm[None]).cuda(), None, S)
    crops, tforms, ok = crops[0].cpu().numpy(), tforms[0].cpu().numpy(), ok[0].cpu().numpy()
    assert ok.tolist() == host_ok.tolist() and 0 in ok and 1 in ok
    for i in range(12):
        if ok[i]:
            want, want_tf = _align_one(ops, frames[0], lm[i], S)
            assert np.array_equal(crops[i], want) and np.array_equal(_bits(tforms[i]), _bits(want_tf)), i
        else:
            assert not crops[i].any() and np.isnan(tforms[i]).all(), i
            with pytest.raises(ValueError):  # align_faces refuses the set
                _align_one(ops, frames[0], lm[i], S)
    assert crops[ok == 1].any()


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 112, 112, 3), (2, 224, 224, 3)])
def test_blur_scores_device_is_blur_scores(ops, shape):
    crops = torch.from_numpy(np.random.default_rng(shape[0]).integers(0, 256, shape, dtype=np.uint8)).cuda()
    crops[1] = 0
    got = ops.blur_scores_device(crops)
    assert got.dtype == torch.float64 and got.device == crops.device
    want = ops.blur_scores(crops)
    assert np.array_equal(_bits(got), _bits(want)) and want[1] == 0.0 and want[0] > 0


# 5 ------------------------------------------------------------------------------------------------
def _chain(det, ops, frames, bufs=None):
    b = bufs or {}
    dets, counts = det.model.detect_device(frames, THRESH, MAX_FACES, b.get("dets"), b.get("counts"))
    crops, tforms, ok = ops.align_device(frames, dets, counts, 112, b.get("crops"), b.get("tforms"), b.get("ok"))
    blur = ops.blur_scores_device(crops.view(-1, 112, 112, 3), b.get("blur"))
    return {"dets": dets, "counts": counts, "crops": crops, "tforms": tforms, "ok": ok, "blur": blur}


def test_chain_is_capturable_in_a_graph(det, ops, frames):
    """No host hop: one eager warm-up, then the three calls captured on fixed buffers replay on new
    frame contents to the eager results, bit for bit."""
    buf = frames.clone()
    bufs = _chain(det, ops, buf)  # warm-up: the size's tables, the slot buffer, the Winograd filters
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _chain(det, ops, buf, bufs)
    for seed in (78, 79):
        new = _noise_frames(seed)
        want = {k: v.clone() for k, v in _chain(det, ops, new).items()}
        buf.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        counts = want["counts"].cpu().numpy()
        assert np.array_equal(bufs["counts"].cpu().numpy(), counts) and counts.max() > 0
        for f, c in enumerate(counts):  # rows past the count are not written
            assert torch.equal(bufs["dets"][f, :min(c, MAX_FACES)].view(torch.int32),
                               want["dets"][f, :min(c, MAX_FACES)].view(torch.int32))
        assert torch.equal(bufs["ok"], want["ok"]) and torch.equal(bufs["crops"], want["crops"])
        assert np.array_equal(_bits(bufs["tforms"]), _bits(want["tforms"]))
        assert np.array_equal(_bits(bufs["blur"]), _bits(want["blur"]))


# 6 ------------------------------------------------------------------------------------------------
def test_torch_ops_are_the_handle_methods(det, ops, frames):
    from facerecognitionpipeline_amd import torch_ops
    hid = torch_ops.register(det.model)
    try:
        want = _chain(det, ops, frames)
        dets, counts = torch.ops.frhip.detect(frames, hid, THRESH, MAX_FACES)
        crops, tforms, ok = torch.ops.frhip.align_detections(frames, dets, counts, 112)
        blur = torch.ops.frhip.blur_scores(crops.flatten(0, 1))
    finally:
        torch_ops.unregister(hid)
    assert torch.equal(counts, want["counts"]) and torch.equal(dets.view(torch.int32), want["dets"].view(torch.int32))
    assert torch.equal(crops, want["crops"]) and torch.equal(ok, want["ok"])
    assert np.array_equal(_bits(tforms), _bits(want["tforms"])) and np.array_equal(_bits(blur), _bits(want["blur"]))


# 7 ------------------------------------------------------------------------------------------------
def test_recognize_frames_is_recognize_per_frame(det, frames, tmp_path):
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    from facerecognitionpipeline_amd.pipeline import RecognitionPipeline
    emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=32)
    gm = GalleryManager(gallery_path=str(tmp_path / "g" / "s.npz"), device=emb.device, verbose=False)
    rows = np.random.default_rng(5).standard_normal((16, 512)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    for i, e in enumerate(rows):
        gm.add_student(f"S{i}", f"N{i}", e)
    loose = {"min_det_score": 0.0, "min_face_size": 0, "max_yaw": 1e9, "max_pitch": 1e9, "max_roll": 1e9,
             "blur_threshold": 0}
    pipe = RecognitionPipeline(emb, gm, loose, detector=det)
    got = pipe.recognize_frames(frames, top_k=3)
    faces = det.detect_batch(frames)
    assert len(got) == N_FRAMES and sum(len(f) for f in faces) >= 2
    n_valid = 0
    for f in range(N_FRAMES):
        want = pipe.recognize(frames[f], faces[f], top_k=3)
        assert len(got[f]) == len(want)
        for g, w in zip(got[f], want):
            assert g["det_score"] == w["det_score"] and g["is_valid"] == w["is_valid"]
            assert np.array_equal(g["bbox"], w["bbox"]) and g["quality_metrics"].keys() == w["quality_metrics"].keys()
            for k, v in w["quality_metrics"].items():
                assert np.array_equal(np.float64(g["quality_metrics"][k]), np.float64(v), equal_nan=True), k
            assert [m[:2] for m in g["matches"]] == [m[:2] for m in w["matches"]]
            # the same crops in another batch: MatchBatcher's bound against match_single_face
            np.testing.assert_allclose([m[2] for m in g["matches"]], [m[2] for m in w["matches"]], atol=1e-6)
            assert g["recognized"] == w["recognized"]
            n_valid += g["is_valid"]
    assert n_valid >= 2
    with pytest.raises(NotImplementedError, match="frame 0"):
        det.det_thresh = 0.0
        try:
            pipe.recognize_frames(frames)
        finally:
            det.det_thresh = THRESH
