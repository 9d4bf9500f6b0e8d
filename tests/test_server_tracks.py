"""CPU-only: the host mirrors of the server session (the server's LiveRecognitionTracker,
FaceRecognitionServer's per-request flow, server_tracks_host, resolve_server_attempts) against the
reference's own outputs in tests/golden/server_tracks.npz (tools/make_golden_server.py);
fr_server_tracks' argument errors; the Flask routes through the test client."""
import base64
import ctypes
import json
import os

import numpy as np
import pytest

from tests import _live_cases as LC
from tests import _server_cases as SC


@pytest.fixture(scope="module")
def fixture_sessions(golden_dir):
    return SC.sessions(np.load(os.path.join(golden_dir, "server_tracks.npz")))


def _mirror(s, out_dir, name, clock):
    from facerecognitionpipeline_amd.face_recognition_server import FaceRecognitionServer
    k = s["kernel"]
    return FaceRecognitionServer(similarity_threshold=s["similarity_threshold"], output_dir=str(out_dir),
                                 session_name=name, max_recognition_attempts=k["max_attempts"],
                                 frame_buffer_size=k["buffer_size"], retry_cooldown=k["retry_cooldown"],
                                 clock=lambda: clock[0], processor=SC.ReplayProcessor(s), embedder=LC.PlanEmbedder(s),
                                 gallery=LC.HostGallery(), verbose=False)


def test_fixture_sessions_are_small(fixture_sessions, golden_dir):
    assert len(fixture_sessions) >= 4 and {s["mode"] for s in fixture_sessions} == {"faces", "frames"}
    assert os.path.getsize(os.path.join(golden_dir, "server_tracks.npz")) < 64 * 1024
    for s in fixture_sessions:
        n = len(s["ids"])
        assert len(s["clocks"]) <= 32 and n <= 256 and s["request_offsets"][-1] == n
        assert s["metrics"].dtype == np.float64 and s["metrics"].shape == (n, 2) and np.isfinite(s["metrics"]).all()
        assert (np.diff(s["clocks"]) >= 0).all() and s["outcome"].shape == (n, 4)
        assert s["statistics"]["total_recognition_attempts"] == len(s["log"])


def test_host_statement_reproduces_the_fixture_and_the_fixture_reaches_every_case(fixture_sessions, tmp_path):
    from facerecognitionpipeline_amd import face_recognition_server as S
    reached = set()
    gallery = LC.HostGallery()
    for k, s in enumerate(fixture_sessions):
        trace = set()
        per_det, order, offsets, keys = SC.grouped(s)
        attempt, best, state, info = S.server_tracks_host(s["metrics"], per_det, order, offsets, trace=trace,
                                                          **s["kernel"])
        assert all(x.dtype == np.int32 for x in (attempt, best, state, info)) and info.shape == (len(keys), 4)
        assert np.array_equal(best >= 0, attempt >= 0) and np.array_equal(state == S.SERVER_ATTEMPT, attempt >= 0), k
        assert not info[:, 3].any() and info[:, 0].sum() == (attempt >= 0).sum(), k
        assert info[:, 1].sum() == (state == S.SERVER_COOLDOWN_SET).sum(), k
        assert info[:, 2].sum() == (state == S.SERVER_RESET).sum(), k
        assert np.array_equal(s["ids"][best[attempt >= 0]], s["ids"][attempt >= 0]), k  # a face of the same track
        log, events = S.resolve_server_attempts(s["ids"].tolist(), attempt, best, LC.recognise_with(s, gallery),
                                                s["similarity_threshold"], s["kernel"]["max_attempts"], trace=trace)
        # the reference's attempts: detection, track, ordinal, best detection, top-3
        assert [[e["det"], e["track"], e["attempt"], e["best"]] for e in log] == s["log"].tolist(), k
        assert [[LC.STUDENT_IDS.index(m[0]) for m in e["matches"]] for e in log] == s["log_top_idx"].tolist(), k
        assert [[m[2] for m in e["matches"]] for e in log] == s["log_top_score"].tolist(), k
        # until its track is recognised, should_recognize's answer is the kernel's state
        first = {}
        for e in events:
            if e["type"] == "recognized":
                first.setdefault(e["track"], e["det"])
        for d in range(len(s["ids"])):
            if d <= first.get(int(s["ids"][d]), len(s["ids"])):
                assert s["outcome"][d, 0] == int(state[d] == S.SERVER_ATTEMPT), (k, d)
                assert s["outcome"][d, 3] == int(state[d] in (S.SERVER_COOLDOWN, S.SERVER_COOLDOWN_SET)), (k, d)
            else:
                assert s["outcome"][d, 0] == 0, (k, d)
        # its attendance follows from the events
        clock = [0.0]
        srv = _mirror(s, tmp_path, f"server_{k}", clock)
        srv.trace = trace
        request_of = np.repeat(np.arange(len(s["clocks"])), np.diff(s["request_offsets"]))
        for r in sorted({int(request_of[e["det"]]) for e in events}):
            request_events = []
            for e in (e for e in events if request_of[e["det"]] == r):
                m = s["metrics"][e["best"]]
                srv.tracker.recognition_attempts[e["track"]] = e["attempt"] % s["kernel"]["max_attempts"] + 1
                face_data = {"det_score": m[0], "quality_metrics": {"blur_score": float(m[1])}}
                request_events.append((e["type"], srv._result_of(e["matches"], e["track"], face_data,
                                                                 "2026-01-01T00:00:00")))
            srv._update_attendance(request_events)
        assert LC.strip(json.loads((tmp_path / f"server_{k}" / "attendance.json").read_text())) == s["attendance"], k
        reached |= trace
    assert reached >= SC.REQUIRED - {"track_twice_in_request", "empty_request"}, sorted(SC.REQUIRED - reached)


def test_tracker_and_the_request_flows_reproduce_the_fixture(fixture_sessions, tmp_path):
    reached = set()
    for k, s in enumerate(fixture_sessions):
        clock = [0.0]
        srv = _mirror(s, tmp_path, f"server_{k}", clock)
        srv.trace = reached
        session = json.loads((tmp_path / f"server_{k}" / "session.json").read_text())
        assert list(session) == ["session_id", "start_time", "end_time", "status", "settings", "statistics"]
        assert session["status"] == "active" and session["settings"] == {
            "similarity_threshold": s["similarity_threshold"], "recognition_interval": 30,
            "max_recognition_attempts": s["kernel"]["max_attempts"]}
        outcome, log = SC.drive(srv, s, lambda seconds: clock.__setitem__(0, seconds))
        assert np.array_equal(outcome, s["outcome"]), k  # per face: answer, attempts, ring length, cooldown
        rows, top_idx, top_score = SC.log_arrays(log)
        assert np.array_equal(rows, s["log"]) and np.array_equal(top_idx, s["log_top_idx"]), k
        assert top_score.tolist() == s["log_top_score"].tolist(), k
        attendance = json.loads((tmp_path / f"server_{k}" / "attendance.json").read_text())
        assert list(attendance) == ["session_id", "last_updated", "recognized", "unrecognized"]
        assert LC.strip(attendance) == s["attendance"], k
        for entry in attendance["recognized"] + attendance["unrecognized"]:
            assert entry["saved_face_path"].endswith("_aligned.png") and os.path.exists(entry["saved_face_path"])
        for entry in attendance["recognized"]:  # the crop beside a recognised face; for whole frames cut on the event
            original = entry["saved_face_path"].replace("_aligned.png", "_original.png")
            assert os.path.exists(original) == (s["mode"] == "frames")
        final = srv.finalize_session()
        assert final["status"] == "completed" and final["end_time"] and "duration_seconds" in final
        assert list(final["statistics"]) == ["total_frames_processed", "total_faces_detected",
                                             "total_recognition_attempts", "unique_students_recognized",
                                             "unrecognized_tracks"]
        assert final["statistics"] == s["statistics"], k
        assert json.loads((tmp_path / f"server_{k}" / "session.json").read_text()) == final
        tr = srv.tracker
        assert len({r["student_id"] for r in tr.recognized_tracks.values()}) == final["statistics"][
            "unique_students_recognized"]
        assert all(len(b) <= s["kernel"]["buffer_size"] for b in tr.track_frame_buffers.values())
        assert tr.client_tracks == {} and all("_frame" not in f for b in tr.track_frame_buffers.values() for f in b)
        if s["mode"] == "frames":
            assert srv.next_track_id == len(s["ids"]) and final["statistics"]["total_faces_detected"] == 0
    assert {"track_twice_in_request", "empty_request", "second_track_higher", "second_track_lower"} <= reached


def test_tracker_methods():
    from facerecognitionpipeline_amd.face_recognition_server import LiveRecognitionTracker
    now = [100.0]
    t = LiveRecognitionTracker(clock=lambda: now[0])
    assert (t.recognition_interval, t.max_attempts, t.buffer_size, t.retry_cooldown) == (30, 3, 10, 10.0)
    assert t.get_best_frame(7) is None and t.get_track_duration(7) == 0.0 and not t.should_recognize(7, 0)
    faces = [{"det_score": d, "quality_metrics": {"blur_score": b}, "n": i}
             for i, (d, b) in enumerate([(0.6, 100.0), (0.7, 50.0)])]
    t.add_frame(7, faces[0], "2026-01-01T00:00:00")
    assert not t.should_recognize(7, 30)           # det_score 0.6 is not over the gate
    t.add_frame(7, faces[1], "2026-01-01T00:00:02")
    assert t.get_best_frame(7)["n"] == 0 and not t.should_recognize(7, 1)  # the 0.6 face is best: no attempt
    assert t.get_track_duration(7) == 2.0
    t.add_frame(8, {"det_score": 0.9, "quality_metrics": {"blur_score": 200.0}}, "2026-01-01T00:00:00")
    assert t.should_recognize(8, 1) and t.should_recognize(8, 17)  # no interval gate
    for _ in range(3):
        t.increment_attempts(8)
    assert 8 in t.track_last_attempt and not t.should_recognize(8, 30)
    assert t.track_cooldowns == {8: 110.0}         # set on the appearance after the last attempt
    now[0] = 109.999
    assert t.is_track_in_cooldown(8) and not t.should_recognize(8, 30) and len(t.track_frame_buffers[8]) == 1
    now[0] = 110.0                                 # exactly at the deadline: the cooldown is over
    assert not t.should_recognize(8, 30)           # ... and the ring went with it
    assert t.track_cooldowns == {} and t.recognition_attempts[8] == 0 and len(t.track_frame_buffers[8]) == 0
    t.set_track_cooldown(9)
    assert t.track_cooldowns == {9: 113.0}
    t.mark_recognized(7, {"name": "x"})
    assert not t.should_recognize(7, 30)


def test_host_statement_limits():
    from facerecognitionpipeline_amd import face_recognition_server as S
    metrics = np.tile(np.array([0.9, 150.0]), (5, 1))
    clock = np.arange(5.0)
    attempt, best, state, info = S.server_tracks_host(metrics, clock, [0, 1, 2, 3, 4], [0, 5])
    assert attempt.tolist() == [0, 1, 2, -1, -1] and best.tolist() == [0, 0, 0, -1, -1]
    assert state.tolist() == [S.SERVER_ATTEMPT] * 3 + [S.SERVER_COOLDOWN_SET, S.SERVER_COOLDOWN]
    assert info.tolist() == [[3, 1, 0, 0]]
    for kw in ({"max_attempts": 0}, {"max_attempts": 17}, {"buffer_size": 0}, {"buffer_size": 65},
               {"retry_cooldown": -1.0}, {"retry_cooldown": float("inf")}, {"det_gate": float("nan")}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            S.server_tracks_host(metrics, clock, [0, 1, 2, 3, 4], [0, 5], **kw)
    for order, off in (([0, 1], [1, 2]), ([0, 1], [0, 1]), ([0, 1, 2], [0, 2, 1, 3])):
        with pytest.raises(ValueError, match="track_offsets"):
            S.server_tracks_host(metrics, clock, order, off)
    with pytest.raises(ValueError, match="clock"):
        S.server_tracks_host(metrics, clock[:4], [0], [0, 1])
    # a non-finite value or a bad index spoils its own track only
    bad = metrics.copy()
    bad[3, 1] = np.nan
    attempt, best, state, info = S.server_tracks_host(bad, clock, [0, 2, 4, 1, 3, 7], [0, 3, 5, 6])
    assert info.tolist() == [[3, 0, 0, 0], [0, 0, 0, S.SERVER_ERR_VALUE], [0, 0, 0, S.SERVER_ERR_ORDER]]
    assert attempt.tolist() == [0, -1, 1, -1, 2] and not state[[1, 3]].any()
    clock2 = clock.copy()
    clock2[0] = np.inf
    assert S.server_tracks_host(metrics, clock2, [0], [0, 1])[3].tolist() == [[0, 0, 0, S.SERVER_ERR_VALUE]]
    # no tracks, a track without appearances
    assert S.server_tracks_host(metrics[:0], clock[:0], [], [0])[3].shape == (0, 4)
    assert S.server_tracks_host(metrics, clock, [1], [0, 0, 1])[3].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]
    order, offsets, keys = S.group_by_track([5, 3, 5, 9, 3])
    assert order.tolist() == [1, 4, 0, 2, 3] and offsets.tolist() == [0, 2, 4, 5] and keys.tolist() == [3, 5, 9]


def test_resolve_server_attempts_cycles_and_an_empty_gallery():
    from facerecognitionpipeline_amd.face_recognition_server import resolve_server_attempts
    calls = []

    def recognise(dets):
        calls.append(list(dets))
        return [[("S", "n", 0.9 if d == 14 else 0.1)] for d in dets]

    # track "a": ordinals 0..3 with max_attempts 2; track "b": recognised at ordinal 1 (best 14), a third dropped
    keys = ["a", "b", "a", "b", "a", "b", "a"]
    log, events = resolve_server_attempts(keys, [0, 0, 1, 1, 2, 2, 3], [10, 11, 12, 14, 10, 11, 12], recognise, 0.5, 2)
    assert calls == [[10, 11], [12, 14], [10], [12]]
    assert [(e["det"], e["attempt"]) for e in log] == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (6, 3)]
    assert [(e["det"], e["type"]) for e in events] == [(2, "unrecognized"), (3, "recognized"), (6, "unrecognized")]
    log, events = resolve_server_attempts([0, 0, 0], [0, 1, -1], [0, 0, -1], lambda dets: [[] for _ in dets], 0.5, 2)
    assert [(e["det"], e["attempt"]) for e in log] == [(0, 0), (1, 1)] and events == []


def test_server_argument_checks(tmp_path):
    from facerecognitionpipeline_amd.face_recognition_server import FaceRecognitionServer
    common = dict(processor=object(), embedder=LC.PlanEmbedder({}), gallery=LC.HostGallery(), output_dir=str(tmp_path),
                  verbose=False)
    for kw, text in (({"max_recognition_attempts": 17}, "max_attempts"), ({"frame_buffer_size": 65}, "buffer_size"),
                     ({"retry_cooldown": -1.0}, "retry_cooldown")):
        with pytest.raises(ValueError, match=text):
            FaceRecognitionServer(**kw, **common)
    srv = FaceRecognitionServer(**common)
    assert srv.session_name is None and srv.tracker is None and srv.perf_monitor is None
    assert (srv.high_quality_crop_size, srv.max_tracking_distance, srv.next_track_id) == (600, 100, 0)
    srv._create_session("s")
    assert srv.tracker.retry_cooldown == 10.0 and sorted(os.listdir(tmp_path / "s")) == [
        "attendance.json", "recognized_faces", "session.json", "snapshots", "unrecognized_faces"]
    with pytest.raises(ValueError, match="one per request"):
        srv.process_requests([([], 1)], [0.0], timestamps=[])
    with pytest.raises(ValueError, match="one entry per frame"):
        srv.process_frames([np.zeros((4, 4, 3), np.uint8)], [1], [], [0.0])
    # a crop over 600 px comes down to 600 on its longer side
    crop = srv._high_quality_crop(np.zeros((900, 1600, 3), np.uint8), [300.0, 300.0, 800.0, 600.0])
    assert crop.shape == (450, 600, 3)  # 800 x 600 with the margin of 150, scaled by 0.75
    assert srv._high_quality_crop(np.zeros((90, 160, 3), np.uint8), [10, 10, 50, 40]).shape == (52, 62, 3)


def test_fr_server_tracks_argument_errors_without_gpu():
    """The argument checks come before the handle, so they are reported for a NULL handle too."""
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    n = 8
    metrics = (ctypes.c_double * (2 * n))()
    clock = (ctypes.c_double * n)()
    order = (ctypes.c_int32 * n)(*range(n))
    outs = {name: (ctypes.c_int32 * n)() for name in ("attempt", "best", "state")}
    info = (ctypes.c_int32 * 8)()

    def call(metrics=metrics, clock=clock, order=order, offsets=(0, 3, 8), n_tracks=2, n_dets=n, max_attempts=3,
             buffer_size=10, retry_cooldown=10.0, det_gate=0.6, info=info, **kw):
        o = dict(outs, **kw)
        off = (ctypes.c_int32 * len(offsets))(*offsets) if offsets is not None else None
        rc = lib.fr_server_tracks(None, metrics, clock, order, off, n_tracks, n_dets, max_attempts, buffer_size,
                                  retry_cooldown, det_gate, o["attempt"], o["best"], o["state"], info, None)
        return rc, lib.fr_last_error(None)

    for kw, text in (({}, b"NULL handle"), ({"metrics": None}, b"NULL buffer"), ({"clock": None}, b"NULL buffer"),
                     ({"order": None}, b"NULL buffer"), ({"offsets": None}, b"NULL buffer"),
                     ({"attempt": None}, b"NULL buffer"), ({"best": None}, b"NULL buffer"),
                     ({"state": None}, b"NULL buffer"), ({"info": None}, b"NULL buffer"),
                     ({"n_tracks": -1}, b"n_tracks"), ({"n_dets": -1}, b"n_dets"),
                     ({"offsets": (1, 3, 8)}, b"track_offsets[0]"),
                     ({"offsets": (0, 5, 3)}, b"track_offsets decrease at track 1"),
                     ({"max_attempts": 0}, b"max_attempts"), ({"max_attempts": 17}, b"max_attempts"),
                     ({"buffer_size": 0}, b"buffer_size"), ({"buffer_size": 65}, b"buffer_size"),
                     ({"retry_cooldown": -0.5}, b"retry_cooldown"), ({"retry_cooldown": float("nan")}, b"retry_cooldown"),
                     ({"retry_cooldown": float("inf")}, b"retry_cooldown"), ({"det_gate": float("nan")}, b"det_gate"),
                     ({"det_gate": float("-inf")}, b"det_gate")):
        rc, msg = call(**kw)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, kw
        assert text in msg, (kw, msg)
    assert not any(any(o) for o in outs.values()) and not any(info)  # nothing was written
    assert call(n_tracks=0, offsets=None)[1] == b"NULL handle"


def test_server_tracks_op_shapes_without_gpu():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        out = torch.ops.frhip.server_tracks(torch.empty(9, 2, dtype=torch.float64), torch.empty(9, dtype=torch.float64),
                                            torch.empty(9, dtype=torch.int32), [0, 4, 4, 9], 3, 10, 10.0, 0.6)
        assert [tuple(x.shape) for x in out] == [(9,), (9,), (9,), (3, 4)]
        assert all(x.dtype == torch.int32 for x in out)
    with pytest.raises(ValueError):  # CPU tensors: there is no CPU fallback
        torch.ops.frhip.server_tracks(torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, dtype=torch.float64),
                                      torch.zeros(1, dtype=torch.int32), [0, 1], 3, 10, 10.0, 0.6)


def test_package_exports_the_server_mirrors():
    import facerecognitionpipeline_amd as pkg
    from facerecognitionpipeline_amd import face_recognition_live as L
    from facerecognitionpipeline_amd import face_recognition_server as S
    assert pkg.FaceRecognitionServer is S.FaceRecognitionServer and pkg.create_app is S.create_app
    assert pkg.ServerRecognitionTracker is S.LiveRecognitionTracker is not L.LiveRecognitionTracker
    assert pkg.LiveRecognitionTracker is L.LiveRecognitionTracker  # that name stays the live loop's
    assert {"FaceRecognitionServer", "ServerRecognitionTracker", "create_app"} <= set(pkg.__all__)
    with pytest.raises(SystemExit):
        S.main(["--use_cpu"])


def test_flask_routes(fixture_sessions, tmp_path):
    pytest.importorskip("flask")
    from facerecognitionpipeline_amd.face_recognition_server import FaceRecognitionServer, create_app
    s = next(s for s in fixture_sessions if s["mode"] == "frames")
    clock = [0.0]
    srv = FaceRecognitionServer(similarity_threshold=s["similarity_threshold"], output_dir=str(tmp_path),
                                clock=lambda: clock[0], processor=SC.ReplayProcessor(s), embedder=LC.PlanEmbedder(s),
                                gallery=LC.HostGallery(), verbose=False)
    client = create_app(srv).test_client()
    assert client.get("/health").get_json() == {"status": "ok", "session": None}
    frame = SC.png_base64(np.full((16, 16, 3), 7, np.uint8))
    for route in ("/process_frame", "/process_faces", "/save_snapshot", "/finalize"):
        answer = client.post(route, json={"frame": frame})
        assert answer.status_code == 400 and "No active session" in answer.get_json()["error"], route
    assert client.post("/init_session", json={}).status_code == 400
    answer = client.post("/init_session", json={"session_name": "class_1"})
    assert answer.status_code == 200 and answer.get_json() == {
        "status": "session_initialized", "session_name": "class_1", "session_dir": str(tmp_path / "class_1")}
    assert client.get("/health").get_json()["session"] == "class_1"
    answer = client.post("/process_frame", json={"frame": frame, "frame_count": 1, "timestamp": SC.stamp(0.0)})
    body = answer.get_json()
    assert answer.status_code == 200, body
    assert sorted(body) == sorted(["frame_count", "faces_detected", "active_tracks", "tracks", "recognized_tracks",
                                   "recognition_attempts", "failed_tracks", "newly_recognized", "newly_failed",
                                   "performance"])  # (jsonify sorts the keys)
    assert body["faces_detected"] == 3 and [t["track_id"] for t in body["tracks"]] == [0, 1, 2]
    assert sorted(body["newly_recognized"]) == ["0", "2"] and body["recognition_attempts"] == {"0": 1, "2": 1}
    assert body["newly_recognized"]["0"]["student_id"] == "S000" and body["performance"] == {}
    faces = [dict(f, track_id=40) for f in SC.client_faces(s, 2)[:1]]
    answer = client.post("/process_faces", json={"faces": faces, "frame_count": 2})
    assert answer.status_code == 200 and answer.get_json()["faces_processed"] == 1
    assert sorted(answer.get_json()) == sorted(["frame_count", "faces_processed", "recognition_events",
                                                "recognized_tracks", "recognition_attempts", "failed_tracks",
                                                "tracks_in_cooldown", "performance"])
    answer = client.post("/save_snapshot", json={"snapshot": frame, "frame_count": 2, "timestamp": "20260101_090000"})
    path = answer.get_json()["path"]
    assert answer.get_json()["saved"] is True and path.endswith("snapshots/snapshot_frame_000002_20260101_090000.png")
    assert open(path, "rb").read() == base64.b64decode(frame)
    # a failure inside a route: 500 with the error and its type, the traceback only when asked for
    answer = client.post("/process_frame", json={"frame": base64.b64encode(b"no image").decode()})
    assert answer.status_code == 500 and set(answer.get_json()) == {"error", "error_type"}
    debug = create_app(srv, debug=True).test_client().post("/save_snapshot", json={"snapshot": 5})
    assert debug.status_code == 500 and set(debug.get_json()) == {"error", "error_type", "traceback"}
    assert client.post("/finalize", json={}).get_json() == {"status": "finalized"}
    session = json.loads((tmp_path / "class_1" / "session.json").read_text())
    assert session["status"] == "completed" and session["statistics"]["total_recognition_attempts"] == 3
    attendance = json.loads((tmp_path / "class_1" / "attendance.json").read_text())
    assert [e["student_id"] for e in attendance["recognized"]] == ["S000", "S001"]
    for entry in attendance["recognized"]:
        assert os.path.exists(entry["saved_face_path"])
        assert os.path.exists(entry["saved_face_path"].replace("_aligned.png", "_original.png"))
