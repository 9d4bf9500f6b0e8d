"""Shared by tools/make_golden.py (capture), test_capture_tracks.py and test_gpu_capture_tracks.py:
the synthetic capture sessions behind tests/golden/capture_tracks.npz, the situations that
fixture must reach, and seeded clips for the launches that are compared with the host mirror.

A detection is given by its doubled centroid (sx, sy) = (x1 + x2, y1 + y2): the box is about 40
wide around it, with x1 + x2 = sx exactly, so odd sx (half-pixel centroids) occur.  Metrics are
(det_score, blur_score, yaw, pitch, roll)."""
import numpy as np

# situations capture_tracks_host(trace=...) names; the fixture has to reach every one of them
REQUIRED = {
    "tie_two_dets_one_track", "tie_two_tracks_one_det", "at_max_distance", "just_under_max_distance",
    "kept_at_max_disappeared", "deleted", "new_id_after_deletion", "delete_then_append", "empty_first",
    "empty_middle", "frame_after_all_died", "more_dets", "more_tracks", "quality_equals_minimum",
    "equal_qualities_in_track", "better_frame_after_completion", "invalid_face", "blur_over_200", "pose_clamped",
    "negative_angle", "partial_saved", "partial_dropped",
}

GOOD = (0.9, 150.0, 5.0, -3.0, 2.0)      # quality about 0.87
BETTER = (0.99, 250.0, 1.0, 0.0, -1.0)   # blur over 200
EDGE = (0.6, 100.0, 30.0, -20.0, 10.0)   # session C's min_quality_score is this one's quality
CLAMPED = (0.9, 400.0, 120.0, 100.0, 95.0)  # pose score below 0 -> 0; quality 0.36 + 0.3
POOR = (0.5, 0.0, 90.0, 90.0, 90.0)      # pose score exactly 0; quality 0.2


def box(sx, sy):
    x1, y1 = sx // 2 - 20, sy // 2 - 20
    return [x1, y1, sx - x1, sy - y1]


def det(sx, sy, m=GOOD, valid=True):
    return (box(sx, sy), tuple(float(v) for v in m), bool(valid))


def just_under(limit):
    """(a, b) with the largest a^2 + b^2 below ``limit``."""
    best = (0, 0, 0)
    for a in range(int(limit ** 0.5) + 1):
        for b in range(a + 1):
            q = a * a + b * b
            if best[0] < q < limit:
                best = (q, a, b)
    return best


def session_a():
    """Ties and the distance edge.  max_distance 80: 4 d^2 < 25600."""
    frames = [
        [],                                                   # empty first frame
        [det(200, 200)],                                      # track 1
        [det(180, 200), det(220, 200)],                       # two detections at q = 400 from track 1
        [det(200, 200)],                                      # tracks 1 and 2 both at q = 400 from it
        [det(200, 360)],                                      # q = 25600 from track 1: distance 80.0, no match
        [det(200, 360), det(200, 200, BETTER), det(220, 200)],  # track 1 is complete: its better frame is ignored
        [det(200, 360), det(220, 200, GOOD, valid=False)],
        [], [], [],                                           # every track dies (max_disappeared 2)
        [det(200, 200)],                                      # a frame after every track has died
        [det(200, 200)],
    ]
    return dict(frames=frames, max_disappeared=2, max_distance=80.0, target_frames=3, min_quality_score=0.5,
                save_partial=0)


def session_b():
    """The disappearance edge, deletion, return and list order.  max_distance 50: 4 d^2 < 10000."""
    P, Q, R = (200, 200), (1000, 200), (2000, 200)
    q, a, b = just_under(10000)
    assert 10000 - q <= 3, q
    Q2 = (Q[0] + a, Q[1] + b)
    frames = [
        [det(*P), det(*Q), det(*R)],
        [det(*P), det(*R)], [det(*P), det(*R)],
        [det(*P), det(*Q), det(*R)],                   # track 2 comes back after exactly max_disappeared frames
        [det(*P), det(*R)], [det(*P), det(*R)], [det(*P), det(*R)],   # one more: track 2 is deleted
        [det(*R), det(*Q), det(*P)],                   # its return opens track 4, behind track 3 in the list
        [det(*P), det(*Q2), det(*R)],                  # just under max_distance from track 4
        [det(*P, valid=False), det(*Q2), det(*R)],
        [det(*P), det(*Q2), det(*R)],
        [det(*P), det(*Q2), det(*R), det(3000, 3000)],  # a one-frame track: saved by save_partial
    ]
    return dict(frames=frames, max_disappeared=2, max_distance=50.0, target_frames=2, min_quality_score=0.5,
                save_partial=1)


def session_c(edge_quality):
    """Quality edges on one steady track, a second track with seeded metrics.  The reference's
    defaults for the tracker's patience; min_quality_score is EDGE's quality."""
    r = np.random.Generator(np.random.PCG64(0xCA97C))
    steady = [(GOOD, False), (POOR, True), (CLAMPED, True), (EDGE, True), (CLAMPED, True), (GOOD, True),
              (BETTER, True), (GOOD, True), (EDGE, True), (POOR, True), (GOOD, False), (BETTER, True),
              (GOOD, True), (GOOD, True)]
    frames = []
    for f, (m, ok) in enumerate(steady):
        dets = [det(400, 400 + 2 * f, m, ok)]
        if 3 <= f <= 8:
            dets.append(det(1000 + 4 * f, 1000, (r.uniform(0.4, 1.0), r.uniform(20, 300), r.uniform(-40, 40),
                                                 r.uniform(-30, 30), r.uniform(-30, 30)), r.random() < 0.8))
        frames.append(dets)
    return dict(frames=frames, max_disappeared=30, max_distance=80.0, target_frames=4,
                min_quality_score=float(edge_quality), save_partial=0)


def random_session(seed, n_frames, max_faces=8, max_disappeared=1, max_distance=50.0, target_frames=3,
                   min_quality_score=0.5, save_partial=0, grid=40, span=12):
    """People on a coarse grid (equal distances are common), walking a step at a time, leaving and
    returning; seeded metrics around the quality threshold."""
    r = np.random.Generator(np.random.PCG64(seed))
    people = [[int(r.integers(0, span)), int(r.integers(0, span))] for _ in range(max_faces)]
    frames = []
    for f in range(n_frames):
        if r.random() < 0.12:
            frames.append([])
            continue
        dets = []
        for p in people:
            p[0] = int(np.clip(p[0] + r.integers(-1, 2), 0, span - 1))
            p[1] = int(np.clip(p[1] + r.integers(-1, 2), 0, span - 1))
            if r.random() < 0.6:
                m = (r.choice([0.5, 0.7, 0.9]), r.choice([40.0, 120.0, 200.0, 260.0]), r.choice([-60.0, 0.0, 20.0]),
                     r.choice([-20.0, 0.0, 45.0]), r.choice([0.0, 10.0, 100.0]))
                dets.append(det(200 + grid * p[0] + int(r.integers(0, 2)), 200 + grid * p[1], m, r.random() < 0.85))
        order = r.permutation(len(dets))
        frames.append([dets[i] for i in order])
    return dict(frames=frames, max_disappeared=max_disappeared, max_distance=max_distance,
                target_frames=target_frames, min_quality_score=min_quality_score, save_partial=save_partial)


def build_sessions(edge_quality):
    return [session_a(), session_b(), session_c(edge_quality),
            random_session(0xD1, 40, save_partial=0), random_session(0xE2, 24, max_disappeared=2, save_partial=1),
            random_session(0xF3, 32, max_faces=6, max_distance=79.99999999999999, target_frames=2)]


def arrays(session):
    """(bbox int32 [n,4], metrics float64 [n,5], valid uint8 [n], frame_offsets int32 [F+1]) of a session."""
    flat = [d for fr in session["frames"] for d in fr]
    bbox = np.array([d[0] for d in flat], dtype=np.int32).reshape(-1, 4)
    metrics = np.array([d[1] for d in flat], dtype=np.float64).reshape(-1, 5)
    valid = np.array([d[2] for d in flat], dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(fr) for fr in session["frames"]])]).astype(np.int32)
    return bbox, metrics, valid, offsets


PARAMS = ("max_disappeared", "max_distance", "target_frames", "min_quality_score", "save_partial")
PER_SESSION = ("bbox", "metrics", "valid", "frame_offsets", "track_id", "quality", "slot", "n_tracks",
               "meta_track_id", "meta_num_frames", "meta_avg_quality", "meta_avg_det_score") + PARAMS


def sessions(fx):
    """The fixture's sessions as dicts of arrays; the settings as plain Python values."""
    out = []
    for s in range(int(fx["n_sessions"])):
        d = {n: fx[f"s{s}_{n}"] for n in PER_SESSION}
        d["params"] = dict(max_disappeared=int(d["max_disappeared"]), max_distance=float(d["max_distance"]),
                           target_frames=int(d["target_frames"]), min_quality_score=float(d["min_quality_score"]),
                           save_partial=bool(d["save_partial"]))
        out.append(d)
    return out


def faces_of(s, f):
    """Frame f of a fixture session as the reference's face dicts (``aligned_face``: a tiny image
    whose red channel is the detection's index in the session)."""
    a, b = int(s["frame_offsets"][f]), int(s["frame_offsets"][f + 1])
    out = []
    for i in range(a, b):
        m = s["metrics"][i]
        img = np.zeros((8, 8, 3), np.uint8)
        img[..., 0] = i % 256
        img[..., 1] = i // 256
        out.append({"index": i, "bbox": s["bbox"][i].astype(int), "det_score": float(m[0]), "aligned_face": img,
                    "quality_metrics": {"blur_score": float(m[1]), "yaw": float(m[2]), "pitch": float(m[3]),
                                        "roll": float(m[4])},
                    "is_valid": bool(s["valid"][i])})
    return out


def drive(tracker, accumulator, s, force_save):
    """CameraFaceCapture.process_frame's loop (face_detection.py:271-283) over a fixture session,
    then the 's' key (:366-370) when ``force_save``.  Returns the per-detection track ids."""
    ids = np.zeros(len(s["valid"]), np.int32)
    for f in range(len(s["frame_offsets"]) - 1):
        for track_id, face in tracker.update(faces_of(s, f)):
            ids[face["index"]] = track_id
            if face["is_valid"]:
                accumulator.add_frame(track_id, face, None)
    if force_save:
        for track_id in list(accumulator.accumulated_frames.keys()):
            if track_id not in accumulator.completed_tracks:
                accumulator.save_track(track_id)
    return ids


def saved_slots(accumulator, n):
    """slot per detection from an accumulator's saved lists (aligned_face carries the index)."""
    slot = np.full(n, -1, np.int32)
    for track_id in accumulator.metadata:
        frames = accumulator.accumulated_frames[track_id][:accumulator.target_frames]
        for rank, fd in enumerate(frames):
            slot[int(fd["aligned_face"][0, 0, 0]) + 256 * int(fd["aligned_face"][0, 0, 1])] = rank
    return slot


def random_clips(seed, n_clips, n_frames=16, max_faces=8, **kw):
    """Seeded clips of one setting for a batched launch: (bbox, metrics, valid, frame_offsets,
    clip_offsets, params)."""
    parts = [random_session(seed + 17 * c, n_frames, max_faces=max_faces, **kw) for c in range(n_clips)]
    arr = [arrays(p) for p in parts]
    fo = np.concatenate([[0]] + [a[3][1:] + sum(len(x[0]) for x in arr[:i]) for i, a in enumerate(arr)]).astype(np.int32)
    co = np.concatenate([[0], np.cumsum([len(a[3]) - 1 for a in arr])]).astype(np.int32)
    params = {k: parts[0][k] for k in PARAMS}
    return (np.concatenate([a[0] for a in arr]), np.concatenate([a[1] for a in arr]),
            np.concatenate([a[2] for a in arr]), fo, co, params)
