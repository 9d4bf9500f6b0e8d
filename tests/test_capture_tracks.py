"""CPU-only: the host mirrors of the capture session (SimpleTracker, FrameAccumulator,
capture_tracks_host) against the reference's own outputs in tests/golden/capture_tracks.npz
(tools/make_golden.py capture); the written folders read back by FaceMatcher._read_track; the
match threshold q_limit; fr_capture_tracks' argument errors."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from tests._capture_cases import REQUIRED, drive, faces_of, saved_slots, sessions
from tests._track_cases import host_matcher


@pytest.fixture(scope="module")
def fixture_sessions(golden_dir):
    return sessions(np.load(os.path.join(golden_dir, "capture_tracks.npz")))


def test_fixture_sessions_are_small(fixture_sessions):
    assert len(fixture_sessions) >= 3
    for s in fixture_sessions:
        n_frames = len(s["frame_offsets"]) - 1
        assert 12 <= n_frames <= 40 and np.diff(s["frame_offsets"]).max() <= 8
        assert s["bbox"].dtype == np.int32 and s["metrics"].dtype == np.float64 and np.isfinite(s["metrics"]).all()


def test_tracker_and_accumulator_reproduce_the_fixture(fixture_sessions, tmp_path):
    from facerecognitionpipeline_amd.face_detection import FrameAccumulator, SimpleTracker
    for k, s in enumerate(fixture_sessions):
        p = s["params"]
        tracker = SimpleTracker(max_disappeared=p["max_disappeared"], max_distance=p["max_distance"])
        acc = FrameAccumulator(target_frames=p["target_frames"], min_quality_score=p["min_quality_score"],
                               output_dir=str(tmp_path / f"s{k}"), verbose=False)
        ids = drive(tracker, acc, s, p["save_partial"])
        assert np.array_equal(ids, s["track_id"]), k
        assert tracker.next_track_id - 1 == int(s["n_tracks"]), k
        quality = np.array([acc.compute_quality_score(f) for fr in range(len(s["frame_offsets"]) - 1)
                            for f in faces_of(s, fr)], dtype=np.float64)
        assert quality.tobytes() == s["quality"].tobytes(), k  # bitwise
        assert np.array_equal(saved_slots(acc, len(ids)), s["slot"]), k
        assert sorted(acc.metadata) == s["meta_track_id"].tolist() == sorted(acc.completed_tracks), k
        for j, tid in enumerate(s["meta_track_id"].tolist()):
            m = acc.metadata[tid]
            assert list(m) == ["track_id", "num_frames", "avg_quality", "avg_det_score", "saved_at", "files"]
            assert m["track_id"] == tid and m["num_frames"] == int(s["meta_num_frames"][j]), (k, tid)
            assert m["avg_quality"] == float(s["meta_avg_quality"][j]), (k, tid)
            assert m["avg_det_score"] == float(s["meta_avg_det_score"][j]), (k, tid)
            assert m["files"] == [f"frame_{i:03d}.jpg" for i in range(m["num_frames"])]
            track_dir = tmp_path / f"s{k}" / f"track_{tid:03d}"
            assert sorted(x.name for x in track_dir.iterdir()) == m["files"] + ["metadata.json"]
            assert json.loads((track_dir / "metadata.json").read_text()) == m
            assert acc.get_status(tid) == "completed"
        assert acc.get_status(10 ** 6) == f"0/{p['target_frames']}"


def test_host_mirror_reproduces_the_fixture_and_the_fixture_reaches_every_case(fixture_sessions):
    from facerecognitionpipeline_amd.face_detection import capture_tracks_host
    reached = set()
    for k, s in enumerate(fixture_sessions):
        trace = set()
        ids, quality, slot, info = capture_tracks_host(s["bbox"], s["metrics"], s["valid"], s["frame_offsets"],
                                                       trace=trace, **s["params"])
        reached |= trace
        assert np.array_equal(ids, s["track_id"]) and ids.dtype == np.int32, k
        assert np.array_equal(slot, s["slot"]) and slot.dtype == np.int32, k
        assert quality.tobytes() == s["quality"].tobytes(), k  # bitwise
        completed = int((s["meta_num_frames"] == s["params"]["target_frames"]).sum())
        assert info == [int(s["n_tracks"]), completed, int(s["meta_num_frames"].sum()), 0], k
        # slot is the frame_NNN number: per saved track 0 .. num_frames - 1, once each
        for tid, n in zip(s["meta_track_id"].tolist(), s["meta_num_frames"].tolist()):
            assert sorted(slot[(ids == tid) & (slot >= 0)].tolist()) == list(range(n)), (k, tid)
        assert set(ids[slot >= 0].tolist()) == set(s["meta_track_id"].tolist()), k
        # avg_quality / avg_det_score of the reference follow from the slots
        for j, tid in enumerate(s["meta_track_id"].tolist()):
            order = sorted(np.flatnonzero((ids == tid) & (slot >= 0)).tolist(), key=lambda i: slot[i])
            assert float(np.mean([float(quality[i]) for i in order])) == float(s["meta_avg_quality"][j]), (k, tid)
            assert float(np.mean([float(s["metrics"][i, 0]) for i in order])) == float(s["meta_avg_det_score"][j])
    assert reached >= REQUIRED, sorted(REQUIRED - reached)


def test_host_mirror_limits():
    from facerecognitionpipeline_amd import face_detection as FD
    good = [0.9, 150.0, 0.0, 0.0, 0.0]
    # 129 detections far apart in one clip (two frames): 129 live tracks
    bbox = np.array([[100 * i, 0, 100 * i + 40, 40] for i in range(129)], np.int32)
    metrics = np.tile(np.array(good), (129, 1))
    ids, quality, slot, info = FD.capture_tracks_host(bbox, metrics, np.ones(129, np.uint8), [0, 128, 129])
    assert info == [0, 0, 0, FD.CAPTURE_ERR_TRACKS] and not ids.any() and (slot == -1).all()
    assert quality.tobytes() == np.full(129, FD.quality_score(*good)).tobytes()
    ids, _q, _s, info = FD.capture_tracks_host(bbox[:128], metrics[:128], np.ones(128, np.uint8), [0, 128])
    assert info[0] == 128 and info[3] == 0 and ids.tolist() == list(range(1, 129))
    far = np.array([[0, 0, (1 << 20) + 1, 40]], np.int32)
    assert FD.capture_tracks_host(far, metrics[:1], [1], [0, 1])[3] == [0, 0, 0, FD.CAPTURE_ERR_COORD]
    far[0, 2] = 1 << 20
    assert FD.capture_tracks_host(far, metrics[:1], [1], [0, 1])[3][3] == 0


def test_written_track_folder_is_read_back_by_the_matcher(fixture_sessions, tmp_path):
    from facerecognitionpipeline_amd.face_detection import FrameAccumulator, SimpleTracker
    s = fixture_sessions[1]  # save_partial: complete and partial tracks
    p = s["params"]
    acc = FrameAccumulator(p["target_frames"], p["min_quality_score"], str(tmp_path / "cap"), verbose=False)
    drive(SimpleTracker(p["max_disappeared"], p["max_distance"]), acc, s, p["save_partial"])
    fm = host_matcher(0.5)
    assert len(acc.metadata) >= 2
    for tid, meta in acc.metadata.items():
        metadata, names, frames = fm._read_track(str(tmp_path / "cap" / f"track_{tid:03d}"))
        assert metadata == meta and names == meta["files"] and len(frames) == meta["num_frames"]
        saved = acc.accumulated_frames[tid][:p["target_frames"]]
        for got, want in zip(frames, saved):  # flat-colour crops: JPEG loss is a few levels at most
            assert got.shape == want["aligned_face"].shape and got.dtype == np.uint8
            assert np.abs(got.astype(int) - want["aligned_face"].astype(int)).max() <= 3


@pytest.mark.parametrize("max_distance", [80, 50, 0.5, 0, 79.99999999999999, 1e-3, 123.456])
def test_q_limit_is_the_references_decision(max_distance):
    """q < q_limit is `sqrt(q / 4.0) < max_distance`, the reference's test on the distance of a pair
    whose doubled centroids differ by q = dx^2 + dy^2, one below, at and one above the limit."""
    from facerecognitionpipeline_amd.face_detection import q_limit
    limit = q_limit(max_distance)
    assert isinstance(limit, int) and limit >= 0
    for q in (limit - 1, limit, limit + 1):
        if q >= 0:
            assert (q < limit) == bool(np.sqrt(np.float64(q) / 4.0) < max_distance), q
            assert (q < limit) == (math.sqrt(q / 4.0) < max_distance), q
    assert {80: 25600, 50: 10000, 0.5: 1, 0: 0, 79.99999999999999: 25600}.get(max_distance, limit) == limit


def test_q_limit_edges():
    from facerecognitionpipeline_amd.face_detection import q_limit
    assert q_limit(-1.0) == 0 and q_limit(float("nan")) == 0
    assert q_limit(float("inf")) == q_limit(1e9) == 1 << 46  # past every q in range (<= 2^45)
    assert q_limit(80.00000000000001) == 25601


def test_capture_tracks_argument_errors_without_gpu():
    """The argument checks come before the handle, so they are reported for a NULL handle too."""
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    n = 8
    bbox = (ctypes.c_int32 * (4 * n))()
    metrics = (ctypes.c_double * (5 * n))()
    valid = (ctypes.c_uint8 * n)()
    track_id = (ctypes.c_int32 * n)()
    quality = (ctypes.c_double * n)()
    slot = (ctypes.c_int32 * n)()
    info = (ctypes.c_int32 * 8)()

    def call(bbox=bbox, metrics=metrics, valid=valid, frame_offsets=(0, 3, 3, 8), clip_offsets=(0, 2, 3), n_clips=2,
             max_disappeared=30, target_frames=12, track_id=track_id, quality=quality, slot=slot, info=info):
        fo = (ctypes.c_int32 * len(frame_offsets))(*frame_offsets) if frame_offsets is not None else None
        co = (ctypes.c_int32 * len(clip_offsets))(*clip_offsets) if clip_offsets is not None else None
        rc = lib.fr_capture_tracks(None, bbox, metrics, valid, fo, co, n_clips, max_disappeared, 80.0, target_frames,
                                   0.5, 0, track_id, quality, slot, info, None)
        return rc, lib.fr_last_error(None)

    big = tuple(range(0, 129 * 33, 129))  # 32 frames of 129 detections
    long_clip = tuple(range(0, 128 * 34, 128))  # 33 frames of 128: 4224 detections in one clip
    for kw, text in (({}, b"NULL handle"),
                     ({"bbox": None}, b"NULL buffer"), ({"metrics": None}, b"NULL buffer"),
                     ({"valid": None}, b"NULL buffer"), ({"frame_offsets": None}, b"NULL buffer"),
                     ({"clip_offsets": None}, b"NULL buffer"), ({"track_id": None}, b"NULL buffer"),
                     ({"quality": None}, b"NULL buffer"), ({"slot": None}, b"NULL buffer"),
                     ({"info": None}, b"NULL buffer"), ({"n_clips": -1}, b"n_clips"),
                     ({"frame_offsets": (1, 3, 3, 8)}, b"frame_offsets[0]"),
                     ({"clip_offsets": (1, 2, 3)}, b"clip_offsets[0]"),
                     ({"frame_offsets": (0, 3, 2, 8)}, b"frame_offsets decrease at frame 1"),
                     ({"clip_offsets": (0, 2, 1)}, b"clip_offsets decrease at clip 1"),
                     ({"frame_offsets": big, "clip_offsets": (0, 32), "n_clips": 1}, b"frame 0 has 129"),
                     ({"frame_offsets": long_clip, "clip_offsets": (0, 33), "n_clips": 1}, b"clip 0 has 4224"),
                     ({"target_frames": 0}, b"target_frames"), ({"target_frames": 65}, b"target_frames"),
                     ({"max_disappeared": -1}, b"max_disappeared")):
        rc, msg = call(**kw)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, kw
        assert text in msg, (kw, msg)
    assert not any(track_id) and not any(info)  # nothing was written
    # no clips: only the handle is missing; and the Python layer checks the frame count, which the
    # C ABI takes from clip_offsets[n_clips]
    assert call(n_clips=0, frame_offsets=None, clip_offsets=None)[1] == b"NULL handle"


def test_capture_tracks_op_shapes_without_gpu():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        out = torch.ops.frhip.capture_tracks(torch.empty(9, 4, dtype=torch.int32), torch.empty(9, 5, dtype=torch.float64),
                                             torch.empty(9, dtype=torch.uint8), [0, 4, 4, 9], [0, 1, 3], 30, 80.0, 12,
                                             0.5, False)
        assert [tuple(x.shape) for x in out] == [(9,), (9,), (9,), (2, 4)]
        assert [x.dtype for x in out] == [torch.int32, torch.float64, torch.int32, torch.int32]
    with pytest.raises(ValueError):  # CPU tensors: there is no CPU fallback
        torch.ops.frhip.capture_tracks(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 5, dtype=torch.float64),
                                       torch.ones(1, dtype=torch.uint8), [0, 1], [0, 1], 30, 80.0, 12, 0.5, False)


def test_package_exports_the_capture_mirrors():
    import facerecognitionpipeline_amd as pkg
    from facerecognitionpipeline_amd import face_detection as FD
    assert pkg.SimpleTracker is FD.SimpleTracker and pkg.FrameAccumulator is FD.FrameAccumulator
    assert pkg.CameraFaceCapture is FD.CameraFaceCapture
    t = FD.SimpleTracker()
    assert (t.max_disappeared, t.max_distance, t.next_track_id) == (30, 50, 1)
    assert t.compute_centroid([0, 0, 3, 4]).tolist() == [1.5, 2.0]
    assert t.compute_iou([0, 0, 2, 2], [1, 1, 3, 3]) == 1 / 7 and t.compute_iou([0, 0, 1, 1], [2, 2, 3, 3]) == 0.0
