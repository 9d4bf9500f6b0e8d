#!/usr/bin/env python3
"""Builds tests/golden/server_tracks.npz from the reference's own server classes.  It runs only where
the reference checkout exists (in the manner of tools/make_golden.py); the tests read the file.

The reference's ``face_recognition_server`` module is imported with ``cv2`` replaced by a small stub
(PNG through PIL, channel flips), ``performance_monitor_server``, ``face_embedder``,
``gallery_manager`` and ``face_recognition`` by empty stand-in modules, and its ``time.time`` and
``datetime.now`` by a scripted clock.  Its ``LiveRecognitionTracker`` and ``FaceRecognitionServer``
(built without the constructor, on the prepared-vector embedder and the host gallery of
tests/_live_cases.py) are driven over the sessions of tests/_server_cases.py: ``process_faces`` with a
no-op ``cleanup_stale_tracks`` attached to the tracker instance (the call raises as committed), and
``process_full_frame``.  Per session the file holds the ids, clocks, metrics and plans, the attempt
log (detection, track, ordinal, best detection, top-3), per face ``should_recognize``'s answer with
the track's attempts, ring length and cooldown flag, ``attendance.json`` without its clock and path
fields, and the statistics.  Before anything is written the builder asserts that
``server_tracks_host`` + ``resolve_server_attempts`` and the mirror classes of
``facerecognitionpipeline_amd.face_recognition_server`` reproduce all of it, and that the sessions
reach every member of ``REQUIRED``.  No reference program text goes into the file.

Usage: ``python tools/make_golden_server.py``"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import tempfile
import types
from datetime import datetime, timedelta

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "server_tracks.npz")
sys.path.insert(0, REPO)

CV2_STUB = '''import io
import numpy as np
from PIL import Image
IMREAD_COLOR = 1
COLOR_RGB2BGR = COLOR_BGR2RGB = 4
IMWRITE_PNG_COMPRESSION = 16
INTER_LANCZOS4 = 4
def cvtColor(img, code):
    assert code == COLOR_RGB2BGR
    return np.ascontiguousarray(img[..., ::-1])
def imdecode(buf, flags):
    with Image.open(io.BytesIO(np.asarray(buf).tobytes())) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])
def imencode(ext, img, params=()):
    assert ext == ".png"
    out = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(out, format="PNG", compress_level=3)
    return True, np.frombuffer(out.getvalue(), np.uint8)
def resize(*a, **k):
    raise RuntimeError("cv2 stub: no crop of the fixture is over 600 px")
'''


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def main() -> None:
    if not os.path.isdir(REF):
        raise SystemExit("reference not present; golden files are generated in the build container only")
    from tests import _live_cases as LC
    from tests import _server_cases as SC
    from facerecognitionpipeline_amd import face_recognition_server as ours
    tmp = tempfile.mkdtemp(prefix="frgolden_server_")
    with open(os.path.join(tmp, "cv2.py"), "w") as f:
        f.write(CV2_STUB)
    sys.path.insert(0, tmp)
    for name, names in (("performance_monitor_server", ["PerformanceMonitorServer"]), ("face_embedder", ["FaceEmbedder"]),
                        ("gallery_manager", ["GalleryManager"]), ("face_recognition", ["FaceProcessor"])):
        mod = types.ModuleType(name)
        for n in names:
            setattr(mod, n, type(n, (), {}))
        sys.modules[name] = mod
    sys.path.append(REF)
    import face_recognition_server as ref  # the reference module

    now = [0.0]

    class ScriptedDatetime(datetime):
        @classmethod
        def now(cls, tz=None):
            return SC.T0 + timedelta(seconds=now[0])

    ref.time = types.SimpleNamespace(time=lambda: now[0])
    ref.datetime = ScriptedDatetime

    def set_clock(seconds):
        now[0] = seconds

    gallery = LC.HostGallery()
    built = SC.build_sessions()
    out = {"n_sessions": np.int32(len(built))}
    reached = set()
    for s, sess in enumerate(built):
        d = SC.as_fixture(sess)
        k = d["kernel"]
        srv = ref.FaceRecognitionServer.__new__(ref.FaceRecognitionServer)
        srv.similarity_threshold = d["similarity_threshold"]
        srv.recognition_interval = 30
        srv.max_recognition_attempts = k["max_attempts"]
        srv.frame_buffer_size = k["buffer_size"]
        srv.output_dir = os.path.join(tmp, "ref_sessions")
        srv.enable_performance_monitoring = srv.enable_gpu_monitoring = False
        srv.model_type, srv.architecture = "adaface", "ir_101"
        srv.embedder, srv.gallery, srv.face_processor = LC.PlanEmbedder(d), gallery, SC.ReplayProcessor(d)
        srv.high_quality_crop_size, srv.max_tracking_distance, srv.next_track_id = 600, 100, 0
        srv.perf_monitor = None
        set_clock(0.0)
        with quiet():
            srv._create_session(f"server_{s}")
        assert srv.tracker.retry_cooldown == 10.0  # _create_session passes none
        srv.tracker.retry_cooldown = k["retry_cooldown"]
        srv.tracker.cleanup_stale_tracks = lambda timeout_seconds=5.0: None
        with quiet():
            outcome, log = SC.drive(srv, d, set_clock)
            srv.finalize_session()
        assert all(e[4] is not None for e in log), s
        rows, top_idx, top_score = SC.log_arrays(log)
        with open(os.path.join(srv.session_dir, "attendance.json")) as f:
            attendance = LC.strip(json.load(f))
        with open(os.path.join(srv.session_dir, "session.json")) as f:
            statistics = json.load(f)["statistics"]
        assert statistics["total_recognition_attempts"] == len(log), s
        if d["mode"] == "frames":
            assert np.array_equal(np.array(sorted(srv.tracker.track_first_seen)), d["ids"]), s
        # the host statement of the kernel's contract is the reference, or the fixture is not written
        trace = set()
        per_det, order, offsets, _keys = SC.grouped(d)
        attempt, best, state, info = ours.server_tracks_host(d["metrics"], per_det, order, offsets, trace=trace, **k)
        h_log, h_events = ours.resolve_server_attempts(d["ids"].tolist(), attempt, best,
                                                       LC.recognise_with(d, gallery), d["similarity_threshold"],
                                                       k["max_attempts"], trace=trace)
        assert [[e["det"], e["track"], e["attempt"], e["best"]] for e in h_log] == rows.tolist(), s
        assert [[m[2] for m in e["matches"]] for e in h_log] == top_score.tolist(), s
        assert [[LC.STUDENT_IDS.index(m[0]) for m in e["matches"]] for e in h_log] == top_idx.tolist(), s
        assert len(h_events) == len(attendance["unrecognized"]) + sum(
            1 for e in log if e[4]["recognized"]), s
        # and the mirror classes give the same outcomes and files
        clock = [0.0]
        mine = ours.FaceRecognitionServer(similarity_threshold=d["similarity_threshold"],
                                          output_dir=os.path.join(tmp, "mirror_sessions"), session_name=f"server_{s}",
                                          max_recognition_attempts=k["max_attempts"], frame_buffer_size=k["buffer_size"],
                                          retry_cooldown=k["retry_cooldown"], clock=lambda: clock[0],
                                          processor=SC.ReplayProcessor(d), embedder=LC.PlanEmbedder(d), gallery=gallery,
                                          verbose=False)
        mine.trace = trace
        m_outcome, m_log = SC.drive(mine, d, lambda seconds: clock.__setitem__(0, seconds))
        assert np.array_equal(m_outcome, outcome), s
        assert sorted(e[:4] for e in m_log) == sorted(e[:4] for e in log), s
        with open(os.path.join(mine.session_dir, "attendance.json")) as f:
            assert LC.strip(json.load(f)) == attendance, s
        assert mine.finalize_session()["statistics"] == statistics, s
        reached |= trace
        for name, v in (("log", rows), ("log_top_idx", top_idx), ("log_top_score", top_score), ("outcome", outcome),
                        ("attendance", np.array(json.dumps(attendance))),
                        ("statistics", np.array(json.dumps(statistics))), ("mode", np.array(d["mode"])),
                        ("max_attempts", np.int32(k["max_attempts"])), ("buffer_size", np.int32(k["buffer_size"])),
                        ("retry_cooldown", np.float64(k["retry_cooldown"])),
                        ("similarity_threshold", np.float64(d["similarity_threshold"]))):
            d[name] = v
        for name in SC.PER_SESSION:
            out[f"s{s}_{name}"] = d[name]
        print("server session", s, d["mode"], "requests", len(d["clocks"]), "detections", len(d["ids"]), "attempts",
              len(log), "recognized", len(attendance["recognized"]), "unrecognized", len(attendance["unrecognized"]),
              info[:, :3].sum(axis=0).tolist(), sorted(trace))
    assert reached >= SC.REQUIRED, sorted(SC.REQUIRED - reached)
    np.savez_compressed(OUT, **out)
    print("server", len(built), "sessions;", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
