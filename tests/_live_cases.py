"""Shared by tools/make_golden.py (live), test_live_tracks.py and test_gpu_live_tracks.py: the
synthetic live sessions behind tests/golden/live_tracks.npz, the situations that fixture must
reach, the stand-ins that drive a ``LiveFaceRecognition`` (the reference's or ours) over them, and
seeded clips for the launches that are compared with the host statement.

A detection is given by its doubled centroid (sx, sy) = (x1 + x2, y1 + y2) as in _capture_cases,
its metrics (det_score, blur_score) and a plan (student, score): the embedding the stand-in
embedder returns for it scores ``score`` against that student's template and a few hundredths
against the others (all distinct), so the gallery search of every crop is known in advance."""
import json

import numpy as np

from tests._capture_cases import box, just_under

# situations live_tracks_host / resolve_attempts / _update_attendance name in their trace
REQUIRED = {
    "nearest_taken_other_in_range", "tie_two_tracks_one_face", "at_max_distance", "just_under_max_distance",
    "back_after_one_frame_new_id", "empty_first", "empty_middle", "live_order_permuted", "ring_of_one",
    "best_evicted_from_ring", "equal_keys_oldest_wins", "blur_exactly_100", "blur_over_100", "interval_one",
    "attempts_exhausted", "recognized_later_then_silent", "unfinished_track", "second_track_higher",
    "second_track_lower",
}

N_STUDENTS = 5
STUDENT_IDS = [f"S{i:03d}" for i in range(N_STUDENTS)]
STUDENT_NAMES = [f"Student {i}" for i in range(N_STUDENTS)]
SHARP = (0.9, 150.0)     # key 0.9
BEST = (0.99, 250.0)     # blur over 100: key 0.99
EDGE = (0.8, 100.0)      # blur exactly 100: key 0.8
DULL = (0.7, 50.0)       # key 0.35
VOLATILE = ("timestamp", "last_updated", "saved_face_path", "first_seen", "duration_seconds")
SETTINGS = ("max_distance", "recognition_interval", "max_attempts", "buffer_size", "similarity_threshold")
PER_SESSION = ("bbox", "metrics", "frame_offsets", "plan_student", "plan_score", "track_id", "log", "log_top_idx",
               "log_top_score", "attendance", "statistics") + SETTINGS


def det(sx, sy, m=SHARP, student=0, score=0.3):
    return (box(sx, sy), (float(m[0]), float(m[1])), (int(student), float(score)))


def session_a():
    """Assignment: the shared nearest track, the tie, the distance edge, the return, the order.
    max_distance 100: 4 d^2 < 40000."""
    q, a, b = just_under(40000)
    assert q == 39994, q  # the largest sum of two squares under 40000
    frames = [
        [],                                        # empty first frame
        [det(200, 200), det(340, 200)],            # tracks 0 and 1
        [det(230, 200), det(260, 200)],            # both nearest to track 0, track 1 in range of the second: id 2
        [det(245, 200)],                           # tracks 0 and 2 at q = 225: the earlier one (a tick: frame 4)
        [det(245, 400)],                           # q = 40000 from track 0: distance 100.0, no match: id 3
        [det(245 + a, 400 + b)],                   # just under max_distance from track 3
        [],                                        # empty middle frame
        [det(245 + a, 400 + b)],                   # back after one frame: id 4, first seen on a tick (frame 8)
        [det(1000, 1000), det(2000, 1000)],        # ids 5 and 6
        [det(2004, 1000), det(1004, 1000)],        # the same two in the other order: the live list is permuted
        [det(1008, 1000), det(2008, 1000)],
        [det(1008, 1004), det(2008, 1004)],        # frame 12: a tick
    ]
    return dict(frames=frames, max_distance=100.0, recognition_interval=4, max_attempts=3, buffer_size=3,
                similarity_threshold=0.5)


def session_b():
    """Selection and resolution on steady tracks far apart.  Ticks on frames 2, 4, ... (indices 1, 3, ...)."""
    T, U, V, W, Z = (400, 400), (1000, 400), (1600, 400), (2200, 400), (2800, 400)
    t_metrics = [BEST, EDGE, EDGE, DULL, SHARP, SHARP, DULL, DULL, DULL, DULL, DULL, DULL, DULL, DULL]
    # T: attempt 0 at index 1 (ring f0, f1: f0), attempt 1 at index 3 (ring f1..f3: f0 is evicted, f1 and
    # f2 have equal keys) is recognised as student 0 with 0.7; the ticks after it make no attempt
    t_scores = {0: 0.3, 1: 0.7}
    frames = []
    for f in range(14):
        dets = [det(*T, t_metrics[f], 0, t_scores.get(f, 0.25)),
                det(*U, SHARP if f % 2 else DULL, 1, 0.3 + 0.01 * f)]       # U: three failures: unrecognized
        if 4 <= f <= 8:
            dets.append(det(*V, SHARP, 0, 0.9))     # V: student 0 again, higher than T's 0.7
        if 6 <= f <= 9:
            dets.append(det(*W, SHARP, 0, 0.6))     # W: student 0 again, lower
        if f >= 11:
            dets.append(det(*Z, SHARP, 2, 0.4))     # Z: first seen on a tick; two failures when the clip ends
        frames.append(dets)
    return dict(frames=frames, max_distance=100.0, recognition_interval=2, max_attempts=3, buffer_size=3,
                similarity_threshold=0.5)


def random_session(seed, n_frames, max_faces=8, max_distance=100.0, recognition_interval=3, max_attempts=2,
                   buffer_size=4, similarity_threshold=0.5, grid=120, span=10):
    """People on a coarse grid (equal distances are common), walking a step at a time, leaving and
    returning; metrics from a few values (equal keys are common); each person is one student with a
    seeded score per frame."""
    r = np.random.Generator(np.random.PCG64(seed))
    people = [[int(r.integers(0, span)), int(r.integers(0, span)), int(r.integers(0, N_STUDENTS))]
              for _ in range(max_faces)]
    frames = []
    for f in range(n_frames):
        if r.random() < 0.1:
            frames.append([])
            continue
        dets = []
        for p in people:
            p[0] = int(np.clip(p[0] + r.integers(-1, 2), 0, span - 1))
            p[1] = int(np.clip(p[1] + r.integers(-1, 2), 0, span - 1))
            if r.random() < 0.7:
                m = (r.choice([0.5, 0.7, 0.9]), r.choice([40.0, 100.0, 120.0, 260.0]))
                score = r.choice([0.2, 0.35, 0.45, 0.55, 0.7, 0.9]) + 0.001 * int(r.integers(0, 20))
                dets.append(det(200 + grid * p[0] + int(r.integers(0, 2)), 200 + grid * p[1], m, p[2], score))
        order = r.permutation(len(dets))
        frames.append([dets[i] for i in order])
    return dict(frames=frames, max_distance=max_distance, recognition_interval=recognition_interval,
                max_attempts=max_attempts, buffer_size=buffer_size, similarity_threshold=similarity_threshold)


def build_sessions():
    return [session_a(), session_b(),
            random_session(0x11FE, 40), random_session(0x22FE, 24, recognition_interval=1, max_attempts=3, buffer_size=2),
            random_session(0x33FE, 32, max_faces=6, max_distance=99.99999999999999, recognition_interval=5,
                           max_attempts=1, buffer_size=10, grid=100)]


def arrays(session):
    """(bbox int32 [n,4], metrics float64 [n,2], frame_offsets int32 [F+1], plan_student int32 [n],
    plan_score float32 [n]) of a session."""
    flat = [d for fr in session["frames"] for d in fr]
    bbox = np.array([d[0] for d in flat], dtype=np.int32).reshape(-1, 4)
    metrics = np.array([d[1] for d in flat], dtype=np.float64).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum([len(fr) for fr in session["frames"]])]).astype(np.int32)
    return (bbox, metrics, offsets, np.array([d[2][0] for d in flat], dtype=np.int32),
            np.array([d[2][1] for d in flat], dtype=np.float32))


def sessions(fx):
    """The fixture's sessions as dicts of arrays; the settings as plain Python values."""
    out = []
    for s in range(int(fx["n_sessions"])):
        d = {n: fx[f"s{s}_{n}"] for n in PER_SESSION}
        d["kernel"] = dict(max_distance=float(d["max_distance"]), recognition_interval=int(d["recognition_interval"]),
                           max_attempts=int(d["max_attempts"]), buffer_size=int(d["buffer_size"]))
        d["similarity_threshold"] = float(d["similarity_threshold"])
        d["attendance"] = json.loads(str(d["attendance"]))
        d["statistics"] = json.loads(str(d["statistics"]))
        out.append(d)
    return out


# ---- the stand-ins ---------------------------------------------------------------------------------
def templates():
    """One basis vector per student."""
    return np.eye(N_STUDENTS, 512, dtype=np.float32)


def embedding_of(student, score, index):
    """A float32 unit vector scoring ``score`` against ``student`` and distinct hundredths against the
    other students."""
    e = np.zeros(512, np.float32)
    for s in range(N_STUDENTS):
        e[s] = score if s == int(student) else 0.01 * (1 + (int(index) + s) % 7)
    e[N_STUDENTS] = np.sqrt(np.float32(1.0) - np.dot(e, e))
    return e


def face_image(index):
    img = np.zeros((8, 8, 3), np.uint8)
    img[..., 0] = index % 256
    img[..., 1] = index // 256
    return img


def index_of(image):
    return int(image[0, 0, 0]) + 256 * int(image[0, 0, 1])


def faces_of(s, f):
    """Frame f of a session as the reference's face dicts."""
    a, b = int(s["frame_offsets"][f]), int(s["frame_offsets"][f + 1])
    return [{"index": i, "bbox": s["bbox"][i].astype(int), "det_score": float(s["metrics"][i, 0]),
             "aligned_face": face_image(i), "landmarks": None, "is_valid": True,
             "quality_metrics": {"blur_score": float(s["metrics"][i, 1])}} for i in range(a, b)]


class ReplayProcessor:
    """``FaceProcessor.process_numpy`` on fixed detections: call i returns the faces of frame i."""

    def __init__(self, s):
        self.s, self.calls = s, 0

    def process_numpy(self, image_rgb, return_all=False):
        faces = faces_of(self.s, self.calls)
        self.calls += 1
        return faces


class PlanEmbedder:
    """``FaceEmbedder.extract_embedding`` returning the prepared vector of the crop's detection."""

    def __init__(self, s):
        self.s = s

    def extract_embedding(self, face_image, normalize=True):
        i = index_of(face_image)
        return embedding_of(self.s["plan_student"][i], self.s["plan_score"][i], i)


class HostGallery:
    """A gallery of ``templates()`` searched on the host: the cosine of the normalised query against
    every template, best first."""

    def __init__(self):
        self.templates = templates()

    def get_all_students(self):
        return dict(zip(STUDENT_IDS, STUDENT_NAMES))

    def search(self, query_embedding, top_k=5):
        q = query_embedding / (np.linalg.norm(query_embedding) + 1e-8)
        sims = np.dot(self.templates, q)
        return [(STUDENT_IDS[i], STUDENT_NAMES[i], float(sims[i])) for i in np.argsort(sims)[::-1][:top_k]]


def drive(live, s):
    """``process_frame`` over every frame of a session on a ``LiveFaceRecognition`` (the reference's or
    ours) whose processor replays the session.  Returns (per-detection track ids, the attempt log
    [(tick detection, track, attempt number, best detection, result or None), ...])."""
    n_frames = len(s["frame_offsets"]) - 1
    ids = np.full(int(s["frame_offsets"][-1]), -1, np.int32)
    log = []
    inner = live._recognize_face

    def recognize(face_data, track_id, *args, **kw):
        tick = live.active_tracks[track_id]["face"]["index"]
        attempt = live.tracker.recognition_attempts.get(track_id, 0)
        result = inner(face_data, track_id, *args, **kw)
        log.append((tick, track_id, attempt, face_data["index"], result))
        return result

    live._recognize_face = recognize
    frame = np.zeros((16, 16, 3), np.uint8)
    for f in range(n_frames):
        out = live.process_frame(frame)
        assert out["frame_count"] == f + 1 and out["faces_detected"] == len(live.active_tracks) == out["active_tracks"]
        for track_id, data in live.active_tracks.items():
            ids[data["face"]["index"]] = track_id
    return ids, log


def strip(x):
    """A JSON value without the fields that depend on the clock or the folder."""
    if isinstance(x, dict):
        return {k: strip(v) for k, v in x.items() if k not in VOLATILE}
    if isinstance(x, list):
        return [strip(v) for v in x]
    return x


def log_arrays(log):
    """(int32 [L,4] tick detection, track, attempt, best; int32 [L,3] top-3 students; float64 [L,3]
    their scores) of an attempt log whose results are the reference's result dicts."""
    rows = np.array([e[:4] for e in log], np.int32).reshape(-1, 4)
    idx = np.array([[STUDENT_IDS.index(m["student_id"]) for m in e[4]["top_matches"]] for e in log],
                   np.int32).reshape(-1, 3)
    score = np.array([[m["score"] for m in e[4]["top_matches"]] for e in log], np.float64).reshape(-1, 3)
    return rows, idx, score


def recognise_with(s, gallery):
    """``resolve_attempts``' callback on the prepared embeddings of session s."""
    return lambda dets: [gallery.search(embedding_of(s["plan_student"][d], s["plan_score"][d], d), top_k=3)
                         for d in dets]


def random_clips(seed, n_clips, n_frames=16, max_faces=8, **kw):
    """Seeded clips of one setting for a batched launch: (bbox, metrics, frame_offsets, clip_offsets,
    kernel settings)."""
    parts = [random_session(seed + 17 * c, n_frames, max_faces=max_faces, **kw) for c in range(n_clips)]
    arr = [arrays(p) for p in parts]
    fo = np.concatenate([[0]] + [a[2][1:] + sum(len(x[0]) for x in arr[:i]) for i, a in enumerate(arr)]).astype(np.int32)
    co = np.concatenate([[0], np.cumsum([len(a[2]) - 1 for a in arr])]).astype(np.int32)
    params = {k: parts[0][k] for k in SETTINGS if k != "similarity_threshold"}
    return np.concatenate([a[0] for a in arr]), np.concatenate([a[1] for a in arr]), fo, co, params
