"""The device quality gate (fr_quality_gate_device) against its numpy statement
(``quality_gate_host``), and the callers that put it behind detect -> align -> blur.

The rule between kernel and statement (tests/_gate_device_inputs.assert_same_gate): every output
bitwise, but yaw and roll within one float32 ulp -- the device's double atan2 / asin and the host's
agree to a few double ulp, so the float32 roundings differ only on a rounding boundary.

Shapes: (n, F) = (1, 1), (3, 8) and (2, 300) -- 300 slots are more than one pass of the 256 threads
and no multiple of 64 -- with counts 0, -1, F and beyond F; the chain tests use the frames, sizes and
detector settings of tests/test_gpu_device_chain.py (the detector's cost is its 640 x 640 canvas).
"""
import numpy as np
import pytest
import torch

from tests import _gate_device_inputs as gi
from tests._gate_inputs import QUALITY_CONFIGS

pytestmark = pytest.mark.gpu

H, W, N_FRAMES, MAX_FACES = 135, 240, 3, 8
THRESH = 0.5
LOOSE = {"min_det_score": 0.0, "min_face_size": 0, "max_yaw": 1e9, "max_pitch": 1e9, "max_roll": 1e9,
         "blur_threshold": 0}


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
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", torch.cuda.current_device()), max_batch=1)


@pytest.fixture(scope="module")
def frames():
    return _noise_frames(77)


def _cfg(config):
    from facerecognitionpipeline_amd.face_recognition import _gate_config
    return _gate_config(config)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _want(dets, counts, ok, blur, config):
    from facerecognitionpipeline_amd.face_recognition import quality_gate_host
    return dict(zip(gi.OUTPUTS, quality_gate_host(dets, counts, ok, blur, config)))


def _run(ops, dets, counts, ok, blur, config):
    return _host(ops.quality_gate_device(_dev(dets), _dev(counts), _dev(ok), _dev(blur), _cfg(config)))


# 1, 2, 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F", [(1, 1), (3, 8), (2, 300)])
@pytest.mark.parametrize("config", [0, 1, 2])
def test_kernel_is_the_statement(ops, n, F, config):
    dets, counts, ok, blur, _ = gi.random_case(n, F, seed=gi.SEED + 17 * F)
    cfg = QUALITY_CONFIGS[config]
    for what, c in (("random counts", counts), ("no counts", None), ("full", np.full(n, F, np.int32)),
                    ("beyond / -1 / 0", np.array([F + 5, -1, 0][:n], np.int32))):
        got = _run(ops, dets, c, ok, blur, cfg)
        gi.assert_same_gate(got, _want(dets, c, ok, blur, cfg), (what, n, F))
        # the packed outputs: totals and tails
        live = np.full(n, F) if c is None else np.clip(c, 0, F)
        total, n_valid = int(live.sum()), int((got["stage"] == 0).sum())
        assert got["frame_offsets"].tolist() == [0] + np.cumsum(live).tolist()
        assert sorted(got["rows"][:total].tolist()) == [f * F + i for f in range(n) for i in range(live[f])]
        assert (got["rows"][total:] == -1).all() and int(got["n_valid"][0]) == n_valid
        assert (got["valid_slots"][n_valid:] == -1).all()
        assert (got["stage"].reshape(-1)[got["valid_slots"][:n_valid]] == 0).all()
        assert ((got["rank"] == -1) == (got["stage"] == 255)).all()
    for what, kw in (("no ok", dict(ok=None, blur=blur)), ("no blur", dict(ok=ok, blur=None)),
                     ("neither", dict(ok=None, blur=None))):
        gi.assert_same_gate(_run(ops, dets, counts, kw["ok"], kw["blur"], cfg),
                            _want(dets, counts, kw["ok"], kw["blur"], cfg), (what, n, F))


def test_gate_outcomes_all_occur_at_300_slots(ops):
    """The (2, 300) case is no empty comparison: every stage occurs and equal keys were planted."""
    dets, counts, ok, blur, planted = gi.random_case(2, 300, seed=gi.SEED + 17 * 300)
    got = _run(ops, dets, counts, ok, blur, {})
    assert set(np.unique(got["stage"]).tolist()) >= {0, 1, 2, 3, 4, 5} and counts[0] == 300
    (f, slots), = planted
    assert np.diff(got["rank"][f, list(slots)]).tolist() == [1, 1]  # one key: neighbours, in slot order


# 3 ------------------------------------------------------------------------------------------------
def test_planted_exact_cases(ops):
    dets, ok, blur, want = gi.planted_case()
    got = _run(ops, dets, None, ok, blur, gi.PLANTED_CONFIG)
    assert got["stage"][0].tolist() == want.tolist()
    gi.assert_same_gate(got, _want(dets, None, ok, blur, gi.PLANTED_CONFIG), "planted")
    m = got["metrics"][0]
    assert m[0, 0] == 0.625 and m[1, 0] < 0.625 and got["stage"][0, 1] == 1
    assert got["bbox"][0, 2].tolist() == [240, 230, 300, 350] and got["bbox"][0, 3, 2] == 299
    assert m[4, 3] == 30.0 and got["stage"][0, 4] == 0       # pitch exactly at its limit: valid
    assert m[5, 3] > 30.0 and got["stage"][0, 5] == 3        # one float32 step beyond
    assert m[6, 4] == 0.0 and np.signbit(m[6, 4]) == False   # dy == 0: roll exactly 0  # noqa: E712
    assert np.isnan(m[7, 2]) and got["stage"][0, 7] == 0     # a NaN angle passes pose, as on the host
    same = [i for i in range(len(want)) if m[i, 0] == 0.75]
    assert len(same) == 3 and np.diff(got["rank"][0, same]).tolist() == [1, 1]  # a stable order
    assert got["stage"][0, 11] == 5 and m[11, 1] == 250.0    # FR_GATE_FIT records every metric
    assert m[13].tolist() == [np.float64(np.float32(0.3)), 0.0, 0.0, 0.0, 0.0]  # the early exit stores zeros
    # without the blur check the blurred slot is valid and the key falls back to score * 1000
    got = _run(ops, dets, None, ok, blur, dict(gi.PLANTED_CONFIG, check_blur=False))
    assert got["stage"][0, 12] == 0 and (got["metrics"][0, :, 1] == 0).all()
    gi.assert_same_gate(got, _want(dets, None, ok, blur, dict(gi.PLANTED_CONFIG, check_blur=False)), "no check")


def test_refused_arguments(ops):
    dets = torch.zeros((1, 8, 15), device="cuda")
    for bad in (dict(max_yaw=float("nan")), dict(min_face_size=float("inf")), dict(blur_threshold=-1e39)):
        with pytest.raises(ValueError):
            ops.quality_gate_device(dets, None, None, None, {**_cfg({}), **bad})
    with pytest.raises(ValueError):
        ops.quality_gate_device(torch.zeros((1, 1025, 15), device="cuda"), None, None, None, _cfg({}))
    with pytest.raises(ValueError):
        ops.quality_gate_device(dets.cpu(), None, None, None, _cfg({}))
    out = ops.quality_gate_device(torch.zeros((0, 8, 15), device="cuda"), None, None, None, _cfg({}))  # a no-op
    assert out["stage"].shape == (0, 8) and out["frame_offsets"].shape == (1,)


# 5 ------------------------------------------------------------------------------------------------
def _chain(det, ops, frames, cfg, bufs=None):
    b = bufs or {}
    dets, counts = det.model.detect_device(frames, THRESH, MAX_FACES, b.get("dets"), b.get("counts"))
    crops, tforms, ok = ops.align_device(frames, dets, counts, 112, b.get("crops"), b.get("tforms"), b.get("ok"))
    blur = ops.blur_scores_device(crops.view(-1, 112, 112, 3), b.get("blur"))
    gate = ops.quality_gate_device(dets, counts, ok, blur, cfg, b.get("gate"))
    return {"dets": dets, "counts": counts, "crops": crops, "tforms": tforms, "ok": ok, "blur": blur, "gate": gate}


def test_chain_with_the_gate_is_capturable_in_a_graph(det, ops, frames):
    """detect -> align -> blur -> gate captured in one graph (no host hop, no allocation in the
    gate) replays on new frame contents to the eager results, bit for bit."""
    cfg = _cfg({"min_det_score": 0.5, "min_face_size": 20, "blur_threshold": 50})
    buf = frames.clone()
    bufs = _chain(det, ops, buf, cfg)  # warm-up: the size's tables, the workspaces
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _chain(det, ops, buf, cfg, bufs)
    for seed in (78, 79):
        new = _noise_frames(seed)
        want = _host(_chain(det, ops, new, cfg)["gate"])
        buf.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        got = _host(bufs["gate"])
        for k in gi.OUTPUTS:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        assert got["frame_offsets"][-1] >= 2


# 6 ------------------------------------------------------------------------------------------------
def test_torch_op_is_the_handle_method(ops):
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401
    dets, counts, ok, blur, _ = gi.random_case(3, 8)
    c = _cfg({})
    want = _host(ops.quality_gate_device(_dev(dets), _dev(counts), _dev(ok), _dev(blur), c))
    limits = [c[k] for k in ("min_det_score", "min_face_size", "max_yaw", "max_pitch", "max_roll", "blur_threshold")]
    got = torch.ops.frhip.quality_gate(_dev(dets), _dev(counts), _dev(ok), _dev(blur), limits, True)
    for k, g in zip(gi.OUTPUTS, got):
        assert np.array_equal(g.cpu().numpy().view(np.uint8), want[k].view(np.uint8)), k
    got = torch.ops.frhip.quality_gate(_dev(dets), None, None, None, limits, True)
    gi.assert_same_gate(dict(zip(gi.OUTPUTS, (g.cpu().numpy() for g in got))), _want(dets, None, None, None, {}), "op")
    with pytest.raises(ValueError):  # CPU tensors: there is no CPU fallback
        torch.ops.frhip.quality_gate(torch.from_numpy(dets), None, None, None, limits, True)


# 7 ------------------------------------------------------------------------------------------------
def _same_metrics(got, want):
    assert list(got) == list(want)
    for k, w in want.items():
        assert type(got[k]) is type(w), (k, type(got[k]), type(w))
        if k == "yaw" and abs(float(w)) > 143.6:  # |ratio| > 0.95: the decision alone is compared
            continue
        if k in ("yaw", "roll"):
            assert abs(float(got[k]) - float(w)) <= 1e-4, (k, got[k], w)
        else:
            assert got[k] == w, (k, got[k], w)


@pytest.mark.parametrize("return_all", [False, True])
def test_process_frames_is_process_numpy_per_frame(det, frames, return_all):
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    # limits inside the range of what the synthetic detector finds in the noise frames (per frame:
    # scores 0.631, 0.629, 0.614, 0.612 and four near 0.607, boxes of 10 px, yaw 80 for the first face and
    # 133 to 148 for the others, roll 20 to 36, blur 1.6 / 2.5 / 4.1 for the first faces), so that slots
    # fail at the score, at the pose and at the blur test, frames 1 and 2 keep one valid face and frame
    # 0 keeps none
    fp = FaceProcessor(output_size=112, detector=det, quality_filter_config={
        "min_det_score": 0.61, "min_face_size": 10, "max_yaw": 100, "max_pitch": 1e9, "max_roll": 40,
        "blur_threshold": 2.0})
    got = fp.process_frames(frames, return_all=return_all)
    host = frames.cpu().numpy()
    assert len(got) == N_FRAMES
    n_faces = 0
    for f in range(N_FRAMES):
        want = fp.process_numpy(host[f], return_all=return_all)
        assert len(got[f]) == len(want), f
        for g, w in zip(got[f], want):
            assert list(g) == list(w)
            assert g["det_score"] == w["det_score"] and g["is_valid"] == w["is_valid"]
            assert g["bbox"].dtype == w["bbox"].dtype and np.array_equal(g["bbox"], w["bbox"])
            assert g["landmarks"].dtype == w["landmarks"].dtype and np.array_equal(g["landmarks"], w["landmarks"])
            assert np.array_equal(g["aligned_face"], w["aligned_face"]) and g["aligned_face"].any()
            _same_metrics(g["quality_metrics"], w["quality_metrics"])
            n_faces += 1
    assert n_faces == (3 * MAX_FACES if return_all else 2)
    if return_all:
        flags = [g["is_valid"] for fr in got for g in fr]
        assert sum(flags) == 2 and {len(g["quality_metrics"]) for fr in got for g in fr} == {1, 5, 6}
    else:
        assert [len(fr) for fr in got] == [0, 1, 1] and all(g["is_valid"] for fr in got for g in fr)
    det.det_thresh = 0.0
    try:
        with pytest.raises(NotImplementedError, match="frame 0"):
            fp.process_frames(frames)
    finally:
        det.det_thresh = THRESH


# 8 ------------------------------------------------------------------------------------------------
def test_recognize_frames_device_gate_is_the_host_gate(det, frames, tmp_path):
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    from facerecognitionpipeline_amd.pipeline import RecognitionPipeline
    emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=32)
    gm = GalleryManager(gallery_path=str(tmp_path / "g" / "s.npz"), device=emb.device, verbose=False)
    rows = np.random.default_rng(5).standard_normal((16, 512)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    for i, e in enumerate(rows):
        gm.add_student(f"S{i}", f"N{i}", e)
    pipe = RecognitionPipeline(emb, gm, LOOSE, detector=det)
    want = pipe.recognize_frames(frames, top_k=3)
    got = pipe.recognize_frames(frames, top_k=3, gate="device")
    assert len(got) == len(want) == N_FRAMES
    n_valid = 0
    for gf, wf in zip(got, want):
        assert len(gf) == len(wf)
        for g, w in zip(gf, wf):
            assert g["det_score"] == w["det_score"] and g["is_valid"] == w["is_valid"]
            assert np.array_equal(g["bbox"], w["bbox"])
            _same_metrics(g["quality_metrics"], w["quality_metrics"])
            assert [m[:2] for m in g["matches"]] == [m[:2] for m in w["matches"]]
            np.testing.assert_allclose([m[2] for m in g["matches"]], [m[2] for m in w["matches"]], atol=1e-6)
            assert g["recognized"] == w["recognized"]
            n_valid += g["is_valid"]
    assert n_valid >= 2
    with pytest.raises(ValueError):
        pipe.recognize_frames(frames, gate="gpu")


# 9 ------------------------------------------------------------------------------------------------
def test_capture_device_chain_is_the_host_chain(det, tmp_path):
    from facerecognitionpipeline_amd.face_detection import CameraFaceCapture
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    clip = _noise_frames(81, n=6)
    results = {}
    for chain in (False, True):
        fp = FaceProcessor(output_size=112, detector=det, quality_filter_config=LOOSE)
        cap = CameraFaceCapture(output_dir=str(tmp_path / str(chain)), skip_frames=1, target_frames_per_person=3,
                                min_quality_score=0.0, processor=fp, verbose=False, device_chain=chain)
        results[chain] = cap.process_clip(clip, save=False, save_partial=True)
    host, dev = results[False], results[True]
    assert [t["track_id"] for t in dev] == [t["track_id"] for t in host] and len(host) >= 2
    apart = 0
    for h, d in zip(host, dev):
        assert len(h["qualities"]) == len(d["qualities"])
        q = np.sort(np.asarray(h["qualities"]))
        if (np.diff(q) > 1e-6).all():  # the order within the track is decided beyond the angles' bound
            assert d["frames"] == h["frames"] and np.array_equal(d["crops"], h["crops"])
            np.testing.assert_allclose(d["qualities"], h["qualities"], atol=1e-6, rtol=0)
            apart += 1
        else:
            np.testing.assert_allclose(np.sort(d["qualities"]), q, atol=1e-6, rtol=0)
            assert sorted(d["frames"]) == sorted(h["frames"])
    assert apart >= 2
