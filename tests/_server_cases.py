"""Shared by tools/make_golden_server.py, test_server_tracks.py and test_gpu_server_tracks.py: the
scripted server sessions behind tests/golden/server_tracks.npz, the situations that fixture must
reach, the stand-ins that drive a ``FaceRecognitionServer`` (the reference's or ours) over them, and
seeded logs for the launches that are compared with the host statement.

A session is a list of requests ``(clock seconds, [face, ...])``; a face is ``(track id, (det_score,
blur_score), (student, score))``: the embedding the stand-in embedder returns for it scores ``score``
against that student's template (tests/_live_cases.py).  Mode "faces" goes through ``process_faces``
with the given client ids, mode "frames" through ``process_full_frame``, where the ids are ignored
and every face gets a fresh one."""
import base64
import io
import json
from datetime import datetime, timedelta

import numpy as np

from tests import _live_cases as LC

# situations server_tracks_host / resolve_server_attempts / FaceRecognitionServer name in their trace
REQUIRED = {
    "fresh_id_per_face", "det_exactly_at_gate", "det_next_double_above_gate", "gated_best_blocks_newer",
    "equal_keys_oldest_wins", "blur_exactly_100", "blur_over_100", "best_evicted_from_ring", "buffer_size_one",
    "attempts_exhausted", "cooldown_set_on_next_appearance", "silent_in_cooldown", "exactly_at_deadline",
    "reset_drops_current_face", "second_cycle_unrecognized", "recognized_later_then_silent", "track_twice_in_request",
    "empty_request", "left_in_cooldown", "retry_cooldown_zero", "second_track_higher", "second_track_lower",
}

GATE = 0.6
OVER = float(np.nextafter(GATE, np.inf))
SHARP = (0.9, 200.0)     # key 0.9
BEST = (0.99, 250.0)     # key 0.99
AT_GATE = (GATE, 100.0)  # key 0.6, det_score not over the gate, blur exactly 100
JUST = (OVER, 100.0)     # the next double: over the gate
DULL = (0.7, 50.0)       # key 0.35
SETTINGS = ("max_attempts", "buffer_size", "retry_cooldown", "similarity_threshold")
PER_SESSION = ("ids", "request_offsets", "clocks", "metrics", "plan_student", "plan_score", "mode", "log",
               "log_top_idx", "log_top_score", "outcome", "attendance", "statistics") + SETTINGS
T0 = datetime(2026, 1, 1, 9, 0, 0)


def face(track, m=SHARP, student=0, score=0.3):
    return (int(track), (float(m[0]), float(m[1])), (int(student), float(score)))


def session_a():
    """Client ids.  Track 7: two cooldown cycles; 8: the gate; 9: recognised on its second attempt; 10:
    equal keys; 12: twice in a request; 8, 13, 14: one student three times."""
    reqs = [
        (0.0, [face(7), face(8, AT_GATE), face(9, SHARP, 3, 0.3), face(10, (0.9, 50.0), 4, 0.2)]),
        (1.0, []),                                                   # an empty request
        (2.0, [face(7), face(8, DULL), face(9, BEST, 3, 0.7),        # 8: the 0.6 face is best and blocks the 0.7
               face(10, (0.45, 100.0), 4, 0.2)]),                    # 10: key 0.45 again: the older one
        (3.0, [face(7, SHARP, 0, 0.35), face(8, DULL), face(9), face(10, (0.45, 300.0), 4, 0.2)]),  # 7: third failure
        (5.0, [face(7), face(8, DULL, 1, 0.3), face(9)]),            # 7: cooldown until 15; 8: the 0.6 face is evicted
        (8.0, [face(7), face(8, JUST, 1, 0.8)]),                     # 7: silent; 8: recognised as student 1
        (15.0, [face(7, BEST)]),                                     # exactly at the deadline: reset, this face goes
        (16.0, [face(7), face(12, SHARP, 2, 0.3), face(12, BEST, 2, 0.9), face(13, SHARP, 1, 0.9)]),
        (17.0, [face(7), face(12), face(12), face(14, SHARP, 1, 0.6)]),
        (18.0, [face(7, SHARP, 0, 0.4)]),                            # the second cycle's third failure
        (19.0, [face(7)]),                                           # cooldown again, and the log ends
    ]
    return dict(requests=reqs, mode="faces", max_attempts=3, buffer_size=3, retry_cooldown=10.0,
                similarity_threshold=0.5)


def session_b():
    """A ring of one, one attempt per cycle and no cooldown time: fail, cooldown set, reset at once."""
    reqs = [(0.0, [face(1)]), (1.0, [face(1)]), (1.0, [face(1, BEST)]), (2.0, [face(1, SHARP, 2, 0.45)]),
            (2.5, [face(1), face(2, DULL, 1, 0.9)]), (2.5, [face(1), face(2, BEST, 1, 0.9)])]
    return dict(requests=reqs, mode="faces", max_attempts=1, buffer_size=1, retry_cooldown=0.0,
                similarity_threshold=0.5)


def session_c():
    """Whole frames: a fresh id per face, so every face over the gate is tried once, on the spot."""
    reqs = [(0.0, [face(0, SHARP, 0, 0.7), face(0, AT_GATE, 1, 0.9), face(0, JUST, 1, 0.8)]),
            (0.1, []),
            (0.2, [face(0, SHARP, 0, 0.9), face(0, DULL, 2, 0.4), face(0, (0.5, 300.0), 2, 0.9)]),
            (0.3, [face(0, BEST, 0, 0.6), face(0, SHARP, 3, 0.2)])]
    return dict(requests=reqs, mode="frames", max_attempts=3, buffer_size=10, retry_cooldown=10.0,
                similarity_threshold=0.5)


def random_log(seed, n_requests, n_tracks=6, mode="faces", max_attempts=2, buffer_size=4, retry_cooldown=2.0,
               similarity_threshold=0.5):
    """A seeded log: a few client ids that come and go (now and then twice in a request), clocks that
    stand still, creep or jump past a cooldown, metrics from a few values (equal keys and the gate are
    common), each track one student with a seeded score per face."""
    r = np.random.Generator(np.random.PCG64(seed))
    student = r.integers(0, LC.N_STUDENTS, n_tracks)
    now, reqs = 0.0, []
    for _ in range(n_requests):
        now += float(r.choice([0.0, 0.25, 0.5, 1.0, 3.0]))
        faces = []
        for t in r.permutation(n_tracks):
            for _twice in range(int(r.choice([0, 1, 1, 1, 2]))):
                m = (r.choice([0.5, GATE, OVER, 0.7, 0.9]), r.choice([40.0, 100.0, 120.0, 260.0]))
                score = r.choice([0.2, 0.35, 0.45, 0.55, 0.7]) + 0.001 * int(r.integers(0, 20))
                faces.append(face(100 + 7 * int(t), m, student[t], score))
        reqs.append((now, faces))
    return dict(requests=reqs, mode=mode, max_attempts=max_attempts, buffer_size=buffer_size,
                retry_cooldown=retry_cooldown, similarity_threshold=similarity_threshold)


def build_sessions():
    return [session_a(), session_b(), session_c(), random_log(0x5E01, 24),
            random_log(0x5E02, 16, n_tracks=4, max_attempts=3, buffer_size=2, retry_cooldown=0.5)]


def arrays(session):
    """(ids int32 [n], request_offsets int32 [R+1], clocks float64 [R], metrics float64 [n,2],
    plan_student int32 [n], plan_score float32 [n]) of a session."""
    flat = [f for _c, faces in session["requests"] for f in faces]
    return (np.array([f[0] for f in flat], dtype=np.int32),
            np.concatenate([[0], np.cumsum([len(faces) for _c, faces in session["requests"]])]).astype(np.int32),
            np.array([c for c, _f in session["requests"]], dtype=np.float64),
            np.array([f[1] for f in flat], dtype=np.float64).reshape(-1, 2),
            np.array([f[2][0] for f in flat], dtype=np.int32), np.array([f[2][1] for f in flat], dtype=np.float32))


def as_fixture(session):
    """The input part of a fixture session, from a session of this module."""
    ids, offsets, clocks, metrics, plan_student, plan_score = arrays(session)
    if session["mode"] == "frames":
        ids = np.arange(len(ids), dtype=np.int32)  # the fresh ids, from next_track_id = 0
    d = dict(ids=ids, request_offsets=offsets, clocks=clocks, metrics=metrics, plan_student=plan_student,
             plan_score=plan_score, mode=session["mode"], similarity_threshold=float(session["similarity_threshold"]))
    d["kernel"] = dict(max_attempts=int(session["max_attempts"]), buffer_size=int(session["buffer_size"]),
                       retry_cooldown=float(session["retry_cooldown"]))
    return d


def sessions(fx):
    """The fixture's sessions as dicts of arrays; the settings as plain Python values."""
    out = []
    for s in range(int(fx["n_sessions"])):
        d = {n: fx[f"s{s}_{n}"] for n in PER_SESSION}
        d["mode"] = str(d["mode"])
        d["kernel"] = dict(max_attempts=int(d["max_attempts"]), buffer_size=int(d["buffer_size"]),
                           retry_cooldown=float(d["retry_cooldown"]))
        d["similarity_threshold"] = float(d["similarity_threshold"])
        d["attendance"] = json.loads(str(d["attendance"]))
        d["statistics"] = json.loads(str(d["statistics"]))
        out.append(d)
    return out


def grouped(s):
    """(clock per detection, order, track_offsets, the distinct ids) of a fixture session."""
    from facerecognitionpipeline_amd.face_recognition_server import group_by_track
    per_det = np.repeat(s["clocks"], np.diff(s["request_offsets"]))
    order, offsets, keys = group_by_track(s["ids"])
    return per_det, order, offsets, keys


# ---- the stand-ins -----------------------------------------------------------------------------------
def png_base64(image):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format="PNG")
    return base64.b64encode(buf.getvalue()).decode("ascii")


def stamp(clock):
    return (T0 + timedelta(seconds=float(clock))).isoformat()


def client_faces(s, r):
    """Request r of a session as the dicts a client posts to ``process_faces``."""
    a, b = int(s["request_offsets"][r]), int(s["request_offsets"][r + 1])
    return [{"index": i, "track_id": int(s["ids"][i]), "bbox": [2.0, 2.0, 10.0, 10.0],
             "det_score": float(s["metrics"][i, 0]), "quality_metrics": {"blur_score": float(s["metrics"][i, 1])},
             "aligned_face_base64": png_base64(LC.face_image(i))} for i in range(a, b)]


class ReplayProcessor:
    """``FaceProcessor.process_numpy`` / ``process_images`` on fixed detections: call i returns the
    faces of request i."""

    def __init__(self, s):
        self.s, self.calls = s, 0

    def process_numpy(self, image_rgb, return_all=False):
        a, b = int(self.s["request_offsets"][self.calls]), int(self.s["request_offsets"][self.calls + 1])
        self.calls += 1
        return [{"bbox": np.array([2, 2, 10, 10], np.float32), "det_score": float(self.s["metrics"][i, 0]),
                 "aligned_face": LC.face_image(i), "landmarks": None, "is_valid": True,
                 "quality_metrics": {"blur_score": float(self.s["metrics"][i, 1])}} for i in range(a, b)]

    def process_images(self, images, return_all=False):
        return [self.process_numpy(image, return_all) for image in images]


def drive(server, s, set_clock):
    """Every request of a session through ``process_faces`` / ``process_full_frame`` of a server (the
    reference's or ours) whose tracker exists; ``set_clock(seconds)`` moves the scripted clock.
    Returns ``(outcome int32 [n,4] = should_recognize's answer, then the track's attempts, ring length
    and cooldown flag right after it; the attempt log [(detection, track, ordinal, best detection,
    result or None), ...])``."""
    tr = server.tracker
    n = int(s["request_offsets"][-1])
    outcome = np.full((n, 4), -1, np.int32)
    current, ordinal, log, results = {}, {}, [], {}
    inner_add, inner_should, inner_inc = tr.add_frame, tr.should_recognize, tr.increment_attempts

    def index_of(face_data):
        return face_data["index"] if "index" in face_data else face_data["track_id"]  # frames: id = detection

    def add_frame(track_id, face_data, timestamp):
        current[track_id] = index_of(face_data)
        return inner_add(track_id, face_data, timestamp)

    def should_recognize(track_id, *a, **kw):
        answer = inner_should(track_id, *a, **kw)
        outcome[current[track_id]] = [int(answer), tr.recognition_attempts.get(track_id, 0),
                                      len(tr.track_frame_buffers[track_id]), int(track_id in tr.track_cooldowns)]
        return answer

    def increment_attempts(track_id):
        k = ordinal.get(track_id, 0)
        ordinal[track_id] = k + 1
        log.append([current[track_id], track_id, k, index_of(tr.get_best_frame(track_id))])
        return inner_inc(track_id)

    tr.add_frame, tr.should_recognize, tr.increment_attempts = add_frame, should_recognize, increment_attempts
    seen = {}
    if hasattr(server, "_result_of"):  # ours: one call per attempt, in attempt order per track
        inner_result = server._result_of

        def result_of(matches, track_id, *a, **kw):
            result = inner_result(matches, track_id, *a, **kw)
            results[(track_id, seen.setdefault(track_id, 0))] = result
            seen[track_id] += 1
            return result

        server._result_of = result_of
    else:
        inner_recognize = server._recognize_face

        def recognize(face_data, track_id):
            result = inner_recognize(face_data, track_id)
            results[(track_id, seen.setdefault(track_id, 0))] = result
            seen[track_id] += 1
            return result

        server._recognize_face = recognize
    frame = np.zeros((16, 16, 3), np.uint8)
    for r, clock in enumerate(s["clocks"]):
        set_clock(float(clock))
        if s["mode"] == "frames":
            out = server.process_full_frame(frame, r + 1, stamp(clock))
            assert out["faces_detected"] == out["active_tracks"] == len(out["tracks"])
        else:
            faces = client_faces(s, r)
            out = server.process_faces(faces, r + 1)
            assert out["faces_processed"] == len(faces)
        assert out["frame_count"] == r + 1 and out["performance"] == {}
    return outcome, [tuple(e) + (results[(e[1], e[2])],) for e in log]


def log_arrays(log):
    """(int32 [L,4] detection, track, ordinal, best; int32 [L,3] top-3 students; float64 [L,3] their
    scores) of an attempt log whose results are result dicts.  In detection order."""
    log = sorted(log, key=lambda e: e[0])
    rows = np.array([e[:4] for e in log], np.int32).reshape(-1, 4)
    idx = np.array([[LC.STUDENT_IDS.index(m["student_id"]) for m in e[4]["top_matches"]] for e in log],
                   np.int32).reshape(-1, 3)
    score = np.array([[m["score"] for m in e[4]["top_matches"]] for e in log], np.float64).reshape(-1, 3)
    return rows, idx, score


def random_tracks(seed, lengths, clock_steps=(0.0, 0.25, 0.5, 1.0, 3.0), det=(0.5, GATE, OVER, 0.7, 0.9),
                  blur=(40.0, 100.0, 120.0, 260.0)):
    """Seeded tracks of the given lengths, interleaved at random into one log: (metrics [n,2], clock
    [n], order, track_offsets).  Clocks never decrease along the log."""
    r = np.random.Generator(np.random.PCG64(seed))
    owner = r.permutation(np.repeat(np.arange(len(lengths)), lengths))
    n = len(owner)
    metrics = np.stack([r.choice(det, n), r.choice(blur, n)], axis=1)
    clock = np.cumsum(r.choice(clock_steps, n)) if n else np.zeros(0)
    order = np.argsort(owner, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return metrics.astype(np.float64).reshape(-1, 2), clock.astype(np.float64), order, offsets
