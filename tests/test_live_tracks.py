"""CPU-only: the host mirrors of the live session (LiveRecognitionTracker, LiveFaceRecognition's
per-frame flow, live_tracks_host, resolve_attempts) against the reference's own outputs in
tests/golden/live_tracks.npz (tools/make_golden.py live); fr_live_tracks' argument errors."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import _live_cases as LC


@pytest.fixture(scope="module")
def fixture_sessions(golden_dir):
    return LC.sessions(np.load(os.path.join(golden_dir, "live_tracks.npz")))


def _mirror(s, out_dir, name):
    from facerecognitionpipeline_amd.face_recognition_live import LiveFaceRecognition
    k = s["kernel"]
    live = LiveFaceRecognition(similarity_threshold=s["similarity_threshold"], output_dir=str(out_dir),
                               session_name=name, recognition_interval=k["recognition_interval"],
                               max_recognition_attempts=k["max_attempts"], frame_buffer_size=k["buffer_size"],
                               processor=LC.ReplayProcessor(s), embedder=LC.PlanEmbedder(s), gallery=LC.HostGallery(),
                               verbose=False)
    live.max_distance = k["max_distance"]
    return live


def test_fixture_sessions_are_small(fixture_sessions):
    assert len(fixture_sessions) >= 3
    for s in fixture_sessions:
        n_frames = len(s["frame_offsets"]) - 1
        assert 12 <= n_frames <= 40 and np.diff(s["frame_offsets"]).max() <= 8
        assert s["bbox"].dtype == np.int32 and s["metrics"].dtype == np.float64 and np.isfinite(s["metrics"]).all()
        assert s["statistics"]["total_recognition_attempts"] == len(s["log"])


def test_host_statement_reproduces_the_fixture_and_the_fixture_reaches_every_case(fixture_sessions, tmp_path):
    from facerecognitionpipeline_amd.face_recognition_live import live_tracks_host, resolve_attempts
    reached = set()
    gallery = LC.HostGallery()
    for k, s in enumerate(fixture_sessions):
        trace = set()
        ids, prev, attempt, best, info = live_tracks_host(s["bbox"], s["metrics"], s["frame_offsets"], trace=trace,
                                                          **s["kernel"])
        assert all(x.dtype == np.int32 for x in (ids, prev, attempt, best))
        assert np.array_equal(ids, s["track_id"]), k
        assert info == [int(ids.max()) + 1, int((attempt >= 0).sum()), len(s["frame_offsets"]) - 1, 0], k
        assert np.array_equal(best >= 0, attempt >= 0), k
        # prev chains stay inside a track and step back one frame
        frame_of = np.repeat(np.arange(len(s["frame_offsets"]) - 1), np.diff(s["frame_offsets"]))
        linked = np.flatnonzero(prev >= 0)
        assert np.array_equal(ids[prev[linked]], ids[linked]) and np.array_equal(frame_of[prev[linked]] + 1,
                                                                                  frame_of[linked]), k
        log, events = resolve_attempts(ids.tolist(), attempt, best, LC.recognise_with(s, gallery),
                                       s["similarity_threshold"], s["kernel"]["max_attempts"], trace=trace)
        # the reference's attempts: tick detection, track, attempt number, best detection, top-3
        assert [[e["det"], e["track"], e["attempt"], e["best"]] for e in log] == s["log"].tolist(), k
        assert [[LC.STUDENT_IDS.index(m[0]) for m in e["matches"]] for e in log] == s["log_top_idx"].tolist(), k
        assert [[m[2] for m in e["matches"]] for e in log] == s["log_top_score"].tolist(), k
        # its attendance follows from the events
        live = _mirror(s, tmp_path, f"live_{k}")
        live.trace = trace
        for f in sorted({int(frame_of[e["det"]]) for e in events}):
            frame_events = []
            for e in (e for e in events if frame_of[e["det"]] == f):
                m = s["metrics"][e["best"]]
                live.tracker.recognition_attempts[e["track"]] = e["attempt"] + 1
                face_data = {"det_score": m[0], "quality_metrics": {"blur_score": float(m[1])}}
                result = live._result_of(e["matches"], e["track"], face_data, "2026-01-01T00:00:00")
                frame_events.append((e["type"], result))
            live._update_attendance(frame_events)
        assert LC.strip(json.loads((tmp_path / f"live_{k}" / "attendance.json").read_text())) == s["attendance"], k
        reached |= trace
    assert reached >= LC.REQUIRED, sorted(LC.REQUIRED - reached)


def test_tracker_and_process_frame_reproduce_the_fixture(fixture_sessions, tmp_path):
    for k, s in enumerate(fixture_sessions):
        live = _mirror(s, tmp_path, f"live_{k}")
        session = json.loads((tmp_path / f"live_{k}" / "session.json").read_text())
        assert list(session) == ["session_id", "start_time", "end_time", "status", "settings", "statistics"]
        assert session["status"] == "active" and session["settings"] == {
            "similarity_threshold": s["similarity_threshold"], "recognition_interval": s["kernel"]["recognition_interval"],
            "max_recognition_attempts": s["kernel"]["max_attempts"]}
        ids, log = LC.drive(live, s)
        assert np.array_equal(ids, s["track_id"]), k
        assert live.next_track_id == int(s["track_id"].max()) + 1
        rows, top_idx, top_score = LC.log_arrays(log)
        assert np.array_equal(rows, s["log"]) and np.array_equal(top_idx, s["log_top_idx"]), k
        assert top_score.tolist() == s["log_top_score"].tolist(), k
        attendance = json.loads((tmp_path / f"live_{k}" / "attendance.json").read_text())
        assert list(attendance) == ["session_id", "last_updated", "recognized", "unrecognized"]
        assert LC.strip(attendance) == s["attendance"], k
        for entry in attendance["recognized"] + attendance["unrecognized"]:
            assert os.path.exists(entry["saved_face_path"]) and entry["duration_seconds"] >= 0
        final = live._finalize_session()
        assert final["status"] == "completed" and final["end_time"] and "duration_seconds" in final
        stats = dict(final["statistics"])
        assert list(stats) == ["total_frames_processed", "total_faces_detected", "total_recognition_attempts",
                               "unique_students_recognized", "unrecognized_tracks", "average_fps"]
        stats.pop("average_fps")
        assert stats == s["statistics"], k
        assert json.loads((tmp_path / f"live_{k}" / "session.json").read_text()) == final
        # the tracker's own record agrees with the attendance
        tr = live.tracker
        assert len({r["student_id"] for r in tr.recognized_tracks.values()}) == stats["unique_students_recognized"]
        assert sum(tr.recognition_attempts.values()) == stats["total_recognition_attempts"]
        assert all(len(b) <= s["kernel"]["buffer_size"] for b in tr.track_frame_buffers.values())


def test_tracker_methods():
    from facerecognitionpipeline_amd.face_recognition_live import LiveRecognitionTracker, selection_key
    t = LiveRecognitionTracker()
    assert (t.recognition_interval, t.max_attempts, t.buffer_size) == (30, 3, 10)
    assert t.get_best_frame(7) is None and t.get_track_duration(7) == 0.0
    faces = [{"det_score": d, "quality_metrics": {"blur_score": b}, "n": i}
             for i, (d, b) in enumerate([(0.9, 50.0), (0.45, 100.0), (0.45, 300.0), (0.2, 100.0)])]
    for i, f in enumerate(faces):
        t.add_frame(7, f, f"2026-01-01T00:00:0{i}")
    assert t.get_best_frame(7)["n"] == 0  # 0.45 three times: the oldest
    assert [selection_key(f["det_score"], f["quality_metrics"]["blur_score"]) for f in faces] == [0.45, 0.45, 0.45, 0.2]
    assert t.get_track_duration(7) == 3.0
    assert not t.should_recognize(7, 29) and t.should_recognize(7, 30) and t.should_recognize(7, 60)
    for _ in range(3):
        t.increment_attempts(7)
    assert not t.should_recognize(7, 30)
    t.mark_recognized(8, {"name": "x"})
    assert not t.should_recognize(8, 30)
    assert t.get_best_frame(9) is None


def test_host_statement_limits():
    from facerecognitionpipeline_amd import face_recognition_live as L
    bbox = np.array([[100 * i, 0, 100 * i + 40, 40] for i in range(129)], np.int32)
    metrics = np.tile(np.array([0.9, 150.0]), (129, 1))
    ids, prev, attempt, best, info = L.live_tracks_host(bbox[:128], metrics[:128], [0, 128], recognition_interval=1)
    assert ids.tolist() == list(range(128)) and info == [128, 128, 1, 0] and best.tolist() == list(range(128))
    with pytest.raises(ValueError, match="128"):
        L.live_tracks_host(bbox, metrics, [0, 129])
    far = np.array([[0, 0, 40, 40], [0, 0, (1 << 20) + 1, 40]], np.int32)
    ids, prev, attempt, best, info = L.live_tracks_host(far, metrics[:2], [0, 1, 2], recognition_interval=1)
    assert info == [0, 0, 0, L.LIVE_ERR_COORD] and not ids.any()
    assert all((x == -1).all() for x in (prev, attempt, best))
    far[1, 2] = 1 << 20
    assert L.live_tracks_host(far, metrics[:2], [0, 1, 2])[4] == [2, 0, 2, 0]
    for kw in ({"recognition_interval": 0}, {"max_attempts": 0}, {"max_attempts": 17}, {"buffer_size": 0},
               {"buffer_size": 65}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            L.live_tracks_host(bbox[:1], metrics[:1], [0, 1], **kw)
    for fo in ([1, 2], [0, 1], [0, 2, 1, 2]):
        with pytest.raises(ValueError):
            L.live_tracks_host(bbox[:2], metrics[:2], fo)
    # max_distance 0 or NaN: nothing ever matches
    same = np.tile(bbox[:1], (3, 1))
    assert L.live_tracks_host(same, metrics[:3], [0, 1, 2, 3], max_distance=0.0)[0].tolist() == [0, 1, 2]
    assert L.live_tracks_host(same, metrics[:3], [0, 1, 2, 3], max_distance=float("nan"))[0].tolist() == [0, 1, 2]
    assert L.live_tracks_host(same, metrics[:3], [0, 1, 2, 3], max_distance=0.5)[0].tolist() == [0, 0, 0]


def test_resolve_attempts_with_an_empty_gallery():
    """No search result: the attempt counts and yields nothing, as the reference's `result is None`."""
    from facerecognitionpipeline_amd.face_recognition_live import resolve_attempts
    log, events = resolve_attempts([0, 0, 0], [0, 1, -1], [0, 0, -1], lambda dets: [[] for _ in dets], 0.5, 2)
    assert [(e["det"], e["attempt"]) for e in log] == [(0, 0), (1, 1)] and events == []


def test_live_tracks_argument_errors_without_gpu():
    """The argument checks come before the handle, so they are reported for a NULL handle too."""
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    n = 8
    bbox = (ctypes.c_int32 * (4 * n))()
    metrics = (ctypes.c_double * (2 * n))()
    outs = {name: (ctypes.c_int32 * n)() for name in ("track_id", "prev", "attempt", "best")}
    info = (ctypes.c_int32 * 8)()

    def call(bbox=bbox, metrics=metrics, frame_offsets=(0, 3, 3, 8), clip_offsets=(0, 2, 3), n_clips=2, interval=30,
             max_attempts=3, buffer_size=10, info=info, **kw):
        o = dict(outs, **kw)
        fo = (ctypes.c_int32 * len(frame_offsets))(*frame_offsets) if frame_offsets is not None else None
        co = (ctypes.c_int32 * len(clip_offsets))(*clip_offsets) if clip_offsets is not None else None
        rc = lib.fr_live_tracks(None, bbox, metrics, fo, co, n_clips, 100.0, interval, max_attempts, buffer_size,
                                o["track_id"], o["prev"], o["attempt"], o["best"], info, None)
        return rc, lib.fr_last_error(None)

    big = tuple(range(0, 129 * 33, 129))  # 32 frames of 129 detections
    long_clip = tuple(range(0, 128 * 41, 128))  # 40 frames of 128: no limit per clip
    for kw, text in (({}, b"NULL handle"),
                     ({"frame_offsets": long_clip, "clip_offsets": (0, 40), "n_clips": 1, "bbox": None}, b"NULL buffer"),
                     ({"bbox": None}, b"NULL buffer"), ({"metrics": None}, b"NULL buffer"),
                     ({"frame_offsets": None}, b"NULL buffer"), ({"clip_offsets": None}, b"NULL buffer"),
                     ({"track_id": None}, b"NULL buffer"), ({"prev": None}, b"NULL buffer"),
                     ({"attempt": None}, b"NULL buffer"), ({"best": None}, b"NULL buffer"),
                     ({"info": None}, b"NULL buffer"), ({"n_clips": -1}, b"n_clips"),
                     ({"frame_offsets": (1, 3, 3, 8)}, b"frame_offsets[0]"),
                     ({"clip_offsets": (1, 2, 3)}, b"clip_offsets[0]"),
                     ({"frame_offsets": (0, 3, 2, 8)}, b"frame_offsets decrease at frame 1"),
                     ({"clip_offsets": (0, 2, 1)}, b"clip_offsets decrease at clip 1"),
                     ({"frame_offsets": big, "clip_offsets": (0, 32), "n_clips": 1}, b"frame 0 has 129"),
                     ({"interval": 0}, b"recognition_interval"), ({"max_attempts": 0}, b"max_attempts"),
                     ({"max_attempts": 17}, b"max_attempts"), ({"buffer_size": 0}, b"buffer_size"),
                     ({"buffer_size": 65}, b"buffer_size")):
        rc, msg = call(**kw)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, kw
        assert text in msg, (kw, msg)
    assert not any(any(o) for o in outs.values()) and not any(info)  # nothing was written
    assert call(n_clips=0, frame_offsets=None, clip_offsets=None)[1] == b"NULL handle"


def test_live_tracks_op_shapes_without_gpu():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        out = torch.ops.frhip.live_tracks(torch.empty(9, 4, dtype=torch.int32), torch.empty(9, 2, dtype=torch.float64),
                                          [0, 4, 4, 9], [0, 1, 3], 100.0, 30, 3, 10)
        assert [tuple(x.shape) for x in out] == [(9,), (9,), (9,), (9,), (2, 4)]
        assert all(x.dtype == torch.int32 for x in out)
    with pytest.raises(ValueError):  # CPU tensors: there is no CPU fallback
        torch.ops.frhip.live_tracks(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.float64),
                                    [0, 1], [0, 1], 100.0, 30, 3, 10)


def test_package_exports_the_live_mirrors():
    import facerecognitionpipeline_amd as pkg
    from facerecognitionpipeline_amd import face_recognition_live as L
    assert pkg.LiveRecognitionTracker is L.LiveRecognitionTracker and pkg.LiveFaceRecognition is L.LiveFaceRecognition
    assert {"LiveRecognitionTracker", "LiveFaceRecognition"} <= set(pkg.__all__)
    with pytest.raises(ValueError, match="max_attempts"):
        L.LiveFaceRecognition(max_recognition_attempts=17, processor=object(), embedder=object(),
                              gallery=LC.HostGallery(), output_dir=os.devnull, verbose=False)
