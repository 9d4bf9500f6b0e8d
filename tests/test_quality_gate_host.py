"""CPU: the contract of the device quality gate (``quality_gate_host``, the numpy statement of
``fr_quality_gate_device``) against the reference's recorded gate, against the per-face
``FaceQualityFilter.is_valid`` loop with ``process_numpy``'s sort, and against the C++ statement the
GPU kernel shares its arithmetic with (``frt_quality_gate_host``).

What is compared how:

* the key set per face (the early exit), the numpy types through ``metrics_from_gate``, det_score,
  face_size, pitch, blur_score, stages and ranks: exactly.  (A detection row holds its score in
  float32, as the detector delivers it, so det_score is the float32 image of the golden's 0.93.)
* yaw and roll: within 1e-4 degrees of numpy's.  The bound is derived, not measured: numpy's float32
  arctan2 / arcsin (a vendor SIMD library on most hosts) stay within 4 ulp of the correctly rounded
  value, which the contract's double-then-round form gives; the degrees product and the doubling
  add at most 1 ulp; an angle of at most 180 degrees has a float32 ulp of at most 1.53e-5 degrees;
  5 x 1.53e-5 = 7.6e-5 < 1e-4.
* yaw only where |ratio| <= 0.95: arcsin's derivative grows without bound towards |ratio| = 1
  (at 0.95 it is 3.2, which the ulp of ratio, a quarter of the angle's, absorbs), so beyond it
  only the decision is compared.  Of the golden set 14 faces lie inside; the one planted beyond the
  yaw limit has its ratio clamped to 1 (asserted).
"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import _gate_device_inputs as gi
from tests._gate_inputs import QUALITY_CONFIGS, detections

ANGLE_TOL = 1e-4


def _rows(dets_list):
    return np.stack([gi.row_of(d["bbox"], d["det_score"], d["landmarks"]) for d in dets_list])


def _ratio(rows):
    """|ratio| of compute_pose_angles for detection rows [..., 15], in float32."""
    ecx = (rows[..., 5] + rows[..., 7]) / np.float32(2)
    dx, dy = rows[..., 7] - rows[..., 5], rows[..., 8] - rows[..., 6]
    with np.errstate(all="ignore"):
        return np.abs((rows[..., 9] - ecx) / np.sqrt(dx * dx + dy * dy))


def _gate(dets, counts, ok, blur, config):
    from facerecognitionpipeline_amd.face_recognition import quality_gate_host
    return dict(zip(gi.OUTPUTS, quality_gate_host(dets, counts, ok, blur, config, dets.shape[1])))


def _check_metrics(qf, got, want, row, blur_checked, n_yaw):
    """One face: ``got`` (metrics_from_gate) against ``want`` (is_valid's dict or the golden's)."""
    assert list(got) == list(want), (list(got), list(want))  # the same early exit
    for k, w in want.items():
        t, v = (w["t"], w["v"]) if isinstance(w, dict) else (type(w).__name__, w)
        assert type(got[k]).__name__ == t, (k, type(got[k]), t)
        if k == "det_score":
            assert got[k] == float(np.float32(v))
        elif k in ("yaw", "roll"):
            if k == "roll" or _ratio(row) <= 0.95:
                assert abs(float(got[k]) - float(v)) <= ANGLE_TOL or (np.isnan(got[k]) and np.isnan(v)), (k, got[k], v)
                n_yaw[0] += k == "yaw"
        else:
            assert float(got[k]) == float(v), (k, got[k], v)


# 1 ------------------------------------------------------------------------------------------------
def test_gate_matches_the_reference_golden(golden_dir):
    """The 15 golden detections as frames of 8 and 7 slots plus an empty frame, under all three
    configurations, with the reference's own blur values."""
    from facerecognitionpipeline_amd.face_recognition import GATE_NOT_LIVE, GATE_VALID, FaceQualityFilter
    records = json.loads(str(np.load(os.path.join(golden_dir, "gate.npz"))["records"]))
    rows15 = _rows(detections())
    assert (_ratio(rows15) <= 0.95).sum() == 14 and _ratio(rows15)[9] > 1
    dets = np.zeros((3, 8, 15), np.float32)
    dets[0], dets[1, :7] = rows15[:8], rows15[8:]
    counts = np.array([8, 7, 0], np.int32)
    seen = set()
    for rec in records:
        if rec["config"] in seen:  # one record per configuration (the gate does not see the frame)
            continue
        seen.add(rec["config"])
        cfg = QUALITY_CONFIGS[rec["config"]]
        qf = FaceQualityFilter(**cfg, device="cpu")
        blur = np.zeros((3, 8))
        for k, want in enumerate(rec["per_face"]):
            blur[k // 8, k % 8] = want["metrics"].get("blur_score", {"v": 0.0})["v"]
        g = _gate(dets, counts, None, blur if qf.check_blur else None, cfg)
        assert (g["stage"][2] == GATE_NOT_LIVE).all() and g["stage"][1, 7] == GATE_NOT_LIVE
        assert g["frame_offsets"].tolist() == [0, 8, 15, 15]
        n_yaw = [0]
        for k, want in enumerate(rec["per_face"]):
            f, i = k // 8, k % 8
            assert (g["stage"][f, i] == GATE_VALID) == want["is_valid"], k
            _check_metrics(qf, qf.metrics_from_gate(g["stage"][f, i], g["metrics"][f, i], g["bbox"][f, i]),
                           want["metrics"], dets[f, i], qf.check_blur, n_yaw)
        assert n_yaw[0] >= 8
    assert seen == {0, 1, 2}


# 4 ------------------------------------------------------------------------------------------------
N_FRAMES, F = 20, 100


@pytest.fixture(scope="module")
def case():
    return gi.random_case(N_FRAMES, F)


def _reference_loop(qf, dets, counts, ok, blur):
    """The per-face is_valid loop and process_numpy's sort -> per frame (valid flags, metrics, order)."""
    from facerecognitionpipeline_amd.face_recognition import FaceDetector
    out = []
    for f in range(dets.shape[0]):
        faces = FaceDetector._faces(dets[f], int(counts[f]))
        res = []
        for i, face in enumerate(faces):
            good, m = qf.is_valid(face, None, None if blur is None else float(blur[f, i]))
            res.append({"i": i, "det_score": face["det_score"], "quality_metrics": m, "is_valid": good})
        order = sorted(res, key=lambda x: x["det_score"] * x["quality_metrics"].get("blur_score", 1000), reverse=True)
        out.append((res, [x["i"] for x in order]))
    return out


@pytest.mark.parametrize("config", [0, 1, 2])
def test_gate_matches_the_is_valid_loop(case, config):
    from facerecognitionpipeline_amd.face_recognition import (GATE_FIT, GATE_POSE, GATE_VALID, FaceQualityFilter,
                                                              _gate_config)
    dets, counts, ok, blur, planted = case
    cfg = QUALITY_CONFIGS[config]
    qf = FaceQualityFilter(**cfg, device="cpu")
    g = _gate(dets, counts, ok, blur if qf.check_blur else None, cfg)
    live = np.arange(F)[None] < counts[:, None]
    assert live.sum() >= 800 and dets.shape[0] * F == 2000
    # the precondition, which excludes nothing: no angle of the statement within 1e-3 degrees of its
    # limit, no two keys of a frame closer than 1e-12 relative unless planted equal
    c = _gate_config(qf)
    posed = live & (g["stage"] != 1) & (g["stage"] != 2)
    for col, lim in ((2, "max_yaw"), (3, "max_pitch"), (4, "max_roll")):
        assert (np.abs(np.abs(g["metrics"][..., col][posed]) - c[lim]) > 1e-3).all(), lim
    key = g["metrics"][..., 0] * np.where(posed & (g["stage"] != GATE_POSE) & qf.check_blur, g["metrics"][..., 1], 1000)
    for f in range(N_FRAMES):
        k = np.sort(key[f, :counts[f]])
        close = np.flatnonzero(np.diff(k) <= 1e-12 * np.abs(k[1:]))
        equal = sum(len(s) - 1 for pf, s in planted if pf == f and len({key[f, i] for i in s}) == 1)
        assert len(close) == equal and (np.diff(k)[close] == 0).all(), (f, close)
    assert any(len({key[pf, i] for i in s}) == 1 for pf, s in planted)  # a stable order shows somewhere
    # stages of every kind occur
    assert set(np.unique(g["stage"][live]).tolist()) >= ({0, 1, 2, 3, 5} | ({4} if qf.check_blur else set()))
    n_yaw, rows_want, valid_want = [0], [], []
    for f, (res, order) in enumerate(_reference_loop(qf, dets, counts, ok, blur if qf.check_blur else None)):
        for x in res:
            i = x["i"]
            stage = g["stage"][f, i]
            assert (stage in (GATE_VALID, GATE_FIT)) == x["is_valid"], (f, i, stage)
            assert (stage == GATE_FIT) == (x["is_valid"] and not ok[f, i])
            _check_metrics(qf, qf.metrics_from_gate(stage, g["metrics"][f, i], g["bbox"][f, i]),
                           x["quality_metrics"], dets[f, i], qf.check_blur, n_yaw)
        assert [int(np.flatnonzero(g["rank"][f] == r)[0]) for r in range(len(order))] == order, f
        assert (g["rank"][f, counts[f]:] == -1).all()
        rows_want += [f * F + i for i in order]
        valid_want += [f * F + i for i in order if g["stage"][f, i] == GATE_VALID]
    assert n_yaw[0] >= 100  # not vacuous: that many yaw values were compared
    total = len(rows_want)
    assert g["rows"][:total].tolist() == rows_want and (g["rows"][total:] == -1).all()
    assert g["frame_offsets"].tolist() == [0] + np.cumsum(counts).tolist()
    assert int(g["n_valid"][0]) == len(valid_want) >= 20
    assert g["valid_slots"][:len(valid_want)].tolist() == valid_want and (g["valid_slots"][len(valid_want):] == -1).all()


# 5 ------------------------------------------------------------------------------------------------
def _cpp_gate(dets, counts, ok, blur, config):
    from facerecognitionpipeline_amd import _lib
    from facerecognitionpipeline_amd.face_recognition import _gate_config
    L = _lib.load()
    L.frt_quality_gate_host.restype = ctypes.c_int
    L.frt_quality_gate_host.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 9
    n, F_ = dets.shape[0], dets.shape[1]
    out = {"stage": np.full((n, F_), 77, np.uint8), "metrics": np.full((n, F_, 5), -1.0),
           "bbox": np.full((n, F_, 4), -7, np.int32), "rank": np.full((n, F_), -7, np.int32),
           "rows": np.full(n * F_, -7, np.int32), "frame_offsets": np.full(n + 1, -7, np.int32),
           "valid_slots": np.full(n * F_, -7, np.int32), "n_valid": np.full(1, -7, np.int32)}
    c = _gate_config(config)
    cfg = _lib.GateConfig(**c)
    keep = [np.ascontiguousarray(dets, np.float32), None if counts is None else np.ascontiguousarray(counts, np.int32),
            None if ok is None else np.ascontiguousarray(ok, np.uint8),
            None if blur is None else np.ascontiguousarray(blur, np.float64)]
    rc = L.frt_quality_gate_host(*(None if a is None else a.ctypes.data for a in keep), n, F_, ctypes.byref(cfg),
                                 *(out[k].ctypes.data for k in gi.OUTPUTS))
    _lib.check(rc)
    return out


@pytest.mark.parametrize("config", [0, 1, 2])
def test_cpp_statement_is_the_numpy_statement(case, config):
    dets, counts, ok, blur, _ = case
    cfg = QUALITY_CONFIGS[config]
    gi.assert_same_gate(_cpp_gate(dets, counts, ok, blur, cfg), _gate(dets, counts, ok, blur, cfg), "random")
    gi.assert_same_gate(_cpp_gate(dets, None, None, None, cfg), _gate(dets, None, None, None, cfg), "all live")


def test_planted_cases_in_both_statements():
    dets, ok, blur, want = gi.planted_case()
    py = _gate(dets, None, ok, blur, gi.PLANTED_CONFIG)
    assert py["stage"][0].tolist() == want.tolist()
    gi.assert_same_gate(_cpp_gate(dets, None, ok, blur, gi.PLANTED_CONFIG), py, "planted")
    m = py["metrics"][0]
    assert m[4, 3] == 30.0 and m[5, 3] > 30.0 and m[6, 4] == 0.0 and np.isnan(m[7, 2])
    same = [i for i in range(len(want)) if m[i, 0] == 0.75]
    assert len(same) == 3 and np.diff(py["rank"][0, same]).tolist() == [1, 1]  # equal keys in slot order


def test_cpp_statement_refuses_bad_arguments():
    dets, ok, blur, _ = gi.planted_case()
    for bad in (dict(max_yaw=float("nan")), dict(blur_threshold=float("inf")), dict(min_det_score=1e39)):
        from facerecognitionpipeline_amd import _lib
        cfg = _lib.GateConfig(**{**{k: float(v) for k, v in gi.DEFAULTS.items() if k != "check_blur"},
                                 "check_blur": 1, **bad})
        L = _lib.load()
        out = {k: np.zeros(64 * 8, np.float64) for k in gi.OUTPUTS}
        L.frt_quality_gate_host.restype = ctypes.c_int
        L.frt_quality_gate_host.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 9
        rc = L.frt_quality_gate_host(dets.ctypes.data, None, None, None, 1, dets.shape[1], ctypes.byref(cfg),
                                     *(out[k].ctypes.data for k in gi.OUTPUTS))
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, bad
    with pytest.raises(ValueError):
        _cpp_gate(np.zeros((1, 1025, 15), np.float32), None, None, None, {})
    with pytest.raises(ValueError):
        _gate(np.zeros((1, 8, 15), np.float32), None, None, None, dict(max_roll=float("inf")))
