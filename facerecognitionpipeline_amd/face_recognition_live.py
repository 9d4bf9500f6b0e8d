"""``LiveRecognitionTracker`` / ``LiveFaceRecognition`` — the reference's live attendance loop
(face_recognition_live.py:18-684): frames in, ``attendance.json`` + ``session.json`` and the saved
face crops of a session folder out.

``LiveRecognitionTracker`` and ``LiveFaceRecognition.process_frame`` are the per-frame host flow with
the reference's names, arguments, dict keys and defaults, on the batch-1 detect / align / embed /
match path.  ``live_tracks_host`` states the track assignment, the recognition gating and the frame
selection of a whole recorded clip in integers; it is the contract of the ``fr_live_tracks`` kernel,
which does the same for many clips (cameras) in one launch.  Whether the reference makes an attempt
depends on earlier results only through "already recognised" and "attempts used up", so a recorded
session replays exactly: the kernel gives every attempt's candidate, ``resolve_attempts`` runs at
most ``max_attempts`` batched embed + match rounds over them, and ``process_clip`` replays the
events through ``_update_attendance`` in (frame, detection) order.  What the reference's server
module copied from this one (the track records, the session files, the attendance merge, the session
close, the resolver) is in attendance_session.py; here is what is the live loop's own.

Notes on parity:

* ``process_frame`` takes the BGR frame ``cv2.VideoCapture`` hands the reference, and so does
  ``process_clip``.  Images are written with PIL (JPEG quality 95); the bytes against
  ``cv2.imwrite`` are UNPINNED, as for ``FrameAccumulator``.
* The tracker compares ``sqrt`` distances in the reference and integers ``q = 4 d^2`` here; the
  order and the threshold are the same (see ``face_detection.q_limit``).  The reference's
  ``max_distance`` is the default argument 100 of ``_simple_track_assignment``; here it is the
  attribute ``max_distance``.
* ``timestamp`` of a result is the frame's timestamp (the reference calls ``datetime.now()`` again
  inside ``_recognize_face``).  ``process_frame(frame, timestamp=...)`` and ``process_clip(...,
  timestamps=...)`` take ISO strings; the default is the wall clock per frame, and for a clip
  ``session_start + i / fps``.
* ``process_clip`` leaves ``tracker.track_frame_buffers`` empty (the crops stay on the device); the
  other tracker dicts end as the per-frame flow leaves them.  A call is one session: no tracker
  state is carried between calls.
* Out of scope: ``run()``'s camera loop, ``_draw_display``, snapshots and the performance monitors
  (``enable_performance_monitoring`` / ``enable_gpu_monitoring`` / ``auto_snapshot`` /
  ``snapshot_interval`` are accepted and ignored; ``perf_monitor`` is None).
"""
from __future__ import annotations

import os
import types
from datetime import datetime, timedelta
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .attendance_session import AttendanceSession, TrackRecords, _resolve, selection_key
from .face_detection import CAPTURE_COORD_MAX, q_limit

# include/frhip.h FR_LIVE_*
LIVE_MAX_FACES = 128
LIVE_MAX_ATTEMPTS = 16
LIVE_MAX_BUFFER = 64
LIVE_ERR_COORD = 2


def _two_squares(q: int) -> bool:
    return any(round((q - a * a) ** 0.5) ** 2 == q - a * a for a in range(int(q ** 0.5) + 1))


def _check_settings(recognition_interval, max_attempts, buffer_size) -> None:
    if int(recognition_interval) < 1:
        raise ValueError("recognition_interval must be >= 1")
    if not 1 <= int(max_attempts) <= LIVE_MAX_ATTEMPTS:
        raise ValueError(f"max_attempts must be in [1, {LIVE_MAX_ATTEMPTS}]")
    if not 1 <= int(buffer_size) <= LIVE_MAX_BUFFER:
        raise ValueError(f"buffer_size must be in [1, {LIVE_MAX_BUFFER}]")


def live_tracks_host(bbox, metrics, frame_offsets, max_distance: float = 100, recognition_interval: int = 30,
                     max_attempts: int = 3, buffer_size: int = 10, trace: Optional[set] = None):
    """What ``fr_live_tracks`` computes for one clip, in plain Python: ``bbox`` int [n,4], ``metrics``
    float64 [n,2] (det_score, blur_score); frame f = detections ``[frame_offsets[f],
    frame_offsets[f+1])``.  Returns ``(track_id int32 [n], prev int32 [n], attempt int32 [n], best
    int32 [n], [tracks opened, candidates, frames, error])``; ``prev`` and ``best`` are detection
    indices of the clip, -1 for none.

    ``trace`` (a set) collects the names of the situations the clip went through: the tests use it
    to show that a fixture reaches them."""
    _check_settings(recognition_interval, max_attempts, buffer_size)
    bbox = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    metrics = np.asarray(metrics, dtype=np.float64).reshape(-1, 2)
    fo = [int(v) for v in np.asarray(frame_offsets).reshape(-1)]
    n = bbox.shape[0]
    if len(fo) < 1 or fo[0] != 0 or fo[-1] != n or any(b < a for a, b in zip(fo[:-1], fo[1:])):
        raise ValueError("frame_offsets must rise from 0 to the number of detections")
    if any(b - a > LIVE_MAX_FACES for a, b in zip(fo[:-1], fo[1:])):
        raise ValueError(f"a frame has more than {LIVE_MAX_FACES} detections")
    ev = trace.add if trace is not None else (lambda name: None)
    track_id = np.zeros(n, np.int32)
    prev, attempt, best = (np.full(n, -1, np.int32) for _ in range(3))
    if n and int(np.abs(bbox).max()) > CAPTURE_COORD_MAX:
        return track_id, prev, attempt, best, [0, 0, 0, LIVE_ERR_COORD]
    key = [selection_key(float(m[0]), float(m[1])) for m in metrics]
    limit = q_limit(max_distance)
    at_limit = limit > 0 and (limit / 4.0) ** 0.5 == float(max_distance)
    # ---- assignment and gating: the live list is the previous frame, [id, sx, sy, ticks]
    live: List[List[int]] = []
    base = 0               # the previous frame's first detection
    dropped: List = []     # (sx, sy) of the tracks the previous frame lost
    next_id = candidates = 0
    for f in range(len(fo) - 1):
        dets = [(int(b[0] + b[2]), int(b[1] + b[3])) for b in bbox[fo[f]:fo[f + 1]]]
        tick = (f + 1) % int(recognition_interval) == 0
        if not dets:
            ev("empty_first" if f == 0 else "empty_middle" if live else "empty_again")
        choice = []
        for sx, sy in dets:
            best_q, pick = limit, -1
            qs = [(t[1] - sx) ** 2 + (t[2] - sy) ** 2 for t in live]
            for tp, q in enumerate(qs):
                if q == limit and at_limit:
                    ev("at_max_distance")
                if q < best_q:  # the first of equal q: the earlier list position
                    best_q, pick = q, tp
            if pick >= 0:
                if qs.count(best_q) > 1:
                    ev("tie_two_tracks_one_face")
                if limit - best_q <= 16 and not any(_two_squares(q) for q in range(best_q + 1, limit)):
                    ev("just_under_max_distance")  # no q between this one and the limit can occur
            choice.append(pick)
        owner: Dict[int, int] = {}
        for di, tp in enumerate(choice):
            if tp >= 0:
                owner.setdefault(tp, di)
        matched = [tp for di, tp in enumerate(choice) if tp >= 0 and owner[tp] == di]
        if any(b < a for a, b in zip(matched[:-1], matched[1:])):
            ev("live_order_permuted")
        new_live = []
        for di, (sx, sy) in enumerate(dets):
            d, tp = fo[f] + di, choice[di]
            fresh = tp < 0 or owner[tp] != di
            if fresh:
                if tp >= 0 and any(q < limit for j, q in enumerate(
                        (t[1] - sx) ** 2 + (t[2] - sy) ** 2 for t in live) if j != tp):
                    ev("nearest_taken_other_in_range")
                if tp < 0 and any((x - sx) ** 2 + (y - sy) ** 2 < limit for x, y in dropped):
                    ev("back_after_one_frame_new_id")
                tid, ticks = next_id, 0
                next_id += 1
            else:
                tid, ticks = live[tp][0], live[tp][3]
                prev[d] = base + tp
            if tick:
                if ticks < int(max_attempts):
                    attempt[d] = ticks
                    ticks += 1
                    candidates += 1
            track_id[d] = tid
            new_live.append([tid, sx, sy, ticks])
        dropped = [(t[1], t[2]) for tp, t in enumerate(live) if tp not in matched]
        live, base = new_live, fo[f]
    # ---- selection: the ring of every candidate
    for d in range(n):
        m = metrics[d]
        if m[1] == 100.0:
            ev("blur_exactly_100")
        if m[1] > 100.0:
            ev("blur_over_100")
        if attempt[d] < 0:
            continue
        ring, at = [d], d
        while len(ring) < int(buffer_size) and prev[at] >= 0:
            at = int(prev[at])
            ring.append(at)
        ring.reverse()  # oldest first, as the deque
        pick = max(ring, key=lambda i: key[i])  # the first of equal keys: the oldest
        best[d] = pick
        if trace is not None:
            if len(ring) == 1 and prev[d] < 0:
                ev("ring_of_one")
            if sum(key[i] == key[pick] for i in ring) > 1:
                ev("equal_keys_oldest_wins")
            older, at = [], ring[0]
            while prev[at] >= 0:
                at = int(prev[at])
                older.append(at)
            if older and max(key[i] for i in older) > key[pick]:
                ev("best_evicted_from_ring")
            if int(recognition_interval) == 1:
                ev("interval_one")
    return track_id, prev, attempt, best, [next_id, candidates, len(fo) - 1, 0]


def resolve_attempts(track_key: Sequence, attempt, best, recognise: Callable[[List[int]], List[List]],
                     similarity_threshold: float, max_attempts: int, trace: Optional[set] = None):
    """The attempts the reference makes, out of ``fr_live_tracks``' speculative candidates.
    ``track_key[d]`` names detection d's track (any hashable), ``attempt`` / ``best`` are the kernel's
    arrays.  Round ``a`` hands the ``best`` detections of the attempt-``a`` candidates whose track is
    not yet recognised to ``recognise(list of detection indices)``, which returns per entry the
    ``gallery.search`` list ``[(student_id, name, score), ...]``.  Returns ``(log, events)``: ``log``
    = the attempts made, ``{'det', 'track', 'attempt', 'best', 'matches'}`` in detection order;
    ``events`` = ``{'det', 'type' ('recognized' | 'unrecognized'), 'track', 'attempt', 'best',
    'matches'}`` in detection order.  An empty ``matches`` (empty gallery) counts as an attempt and
    yields nothing, as in the reference."""
    log, events = _resolve(range(int(max_attempts)), track_key, attempt, best, recognise, similarity_threshold,
                           max_attempts, trace)
    if trace is not None:
        made: Dict = {}
        for e in log:
            made[e["track"]] = max(made.get(e["track"], 0), e["attempt"] + 1)
        recognized = {e["track"] for e in events if e["type"] == "recognized"}
        if any(k not in recognized and count < int(max_attempts) for k, count in made.items()):
            trace.add("unfinished_track")
    return log, events


class LiveRecognitionTracker(TrackRecords):
    """face_recognition_live.py:18-80: the records of every track id ever opened (ids do not come
    back), and the every-N-frames gate."""

    def __init__(self, recognition_interval=30, max_attempts=3, buffer_size=10):
        super().__init__(recognition_interval, max_attempts, buffer_size)

    def should_recognize(self, track_id: int, frame_count: int) -> bool:
        resolved = track_id in self.recognized_tracks
        spent = self.recognition_attempts.get(track_id, 0) >= self.max_attempts
        return not resolved and not spent and frame_count % self.recognition_interval == 0


class LiveFaceRecognition(AttendanceSession):
    """face_recognition_live.py:82-684 without the camera and the window.  ``processor`` (a
    ``FaceProcessor``, or anything with its ``process_numpy``; ``process_clip`` also needs its
    ``detector`` / ``aligner`` / ``quality_filter``), ``embedder`` and ``gallery`` default to the
    reference's settings (:114-147)."""

    def __init__(self, gallery_path="gallery/students.pkl", similarity_threshold=0.5, output_dir="sessions",
                 session_name=None, recognition_interval=30, max_recognition_attempts=3, frame_buffer_size=10,
                 enable_performance_monitoring=True, enable_gpu_monitoring=True, use_gpu=True, model_type="adaface",
                 architecture="ir_101", auto_snapshot=True, snapshot_interval=5.0, model_path=None, device=None,
                 processor=None, embedder=None, gallery=None, verbose: bool = True, device_chain: bool = False):
        self.verbose = verbose
        self.device_chain = bool(device_chain)  # process_clip: CameraFaceCapture's device chain per clip
        self._print("\n" + "=" * 70)
        self._print("INITIALIZING LIVE FACE RECOGNITION SYSTEM")
        self._print("=" * 70)
        self.similarity_threshold = similarity_threshold
        self.recognition_interval = recognition_interval
        self.max_recognition_attempts = max_recognition_attempts
        self.max_distance = 100  # _simple_track_assignment's default argument
        self._load_processor(processor, device)
        self._load_embedder(embedder, architecture, model_path, model_type, device)
        self._load_gallery(gallery, gallery_path)
        self.session_name = session_name or f"session_{datetime.now().strftime('%Y%m%d_%H%M%S')}"
        self.session_dir = os.path.join(output_dir, self.session_name)
        self.perf_monitor = None
        self.auto_snapshot = False
        self.trace: Optional[set] = None  # the tests' record of the situations _update_attendance met
        self.cameras: List["LiveFaceRecognition"] = [self]  # one per clip of the last process_clip call
        self._frame_buffer_size = frame_buffer_size
        _check_settings(recognition_interval, max_recognition_attempts, frame_buffer_size)
        self._start_session()
        self._print("\n" + "=" * 70)
        self._print("System ready!")
        self._print(f"Session: {self.session_name}")
        self._print(f"Output: {self.session_dir}")
        self._print(f"Recognition interval: every {recognition_interval} frames")
        self._print(f"Similarity threshold: {similarity_threshold}")
        self._print("=" * 70 + "\n")

    def _start_session(self) -> None:
        """The session state of the constructor (:173-207): folders, tracker, counters, files."""
        self.active_tracks: Dict[int, Dict] = {}
        self.next_track_id = 0
        self._open_session(LiveRecognitionTracker(recognition_interval=self.recognition_interval,
                                                  max_attempts=self.max_recognition_attempts,
                                                  buffer_size=self._frame_buffer_size))

    def _camera(self, index: int) -> "LiveFaceRecognition":
        """A session of its own under ``session_dir/camera_%02d`` that shares the models."""
        cam = LiveFaceRecognition.__new__(LiveFaceRecognition)
        cam.__dict__.update(self.__dict__)
        cam.session_name = f"{self.session_name}_camera_{index:02d}"
        cam.session_dir = os.path.join(self.session_dir, f"camera_{index:02d}")
        cam.cameras = [cam]
        cam._start_session()
        return cam

    # -- the per-frame flow (:249-414) ------------------------------------------------------
    def _simple_track_assignment(self, faces: List[Dict], max_distance=None):
        """:249-285.  The live tracks are those of the previous call, in its face order.  A face takes
        its nearest live track (the first of equally near ones) when that is nearer than
        ``max_distance`` and no earlier face of this call took it; any other face opens a new id, also
        when a second track is in range.  Tracks no face took are dropped."""
        limit = self.max_distance if max_distance is None else max_distance
        live_ids = list(self.active_tracks)
        live_xy = np.array([[self.active_tracks[t]["x"], self.active_tracks[t]["y"]] for t in live_ids],
                           dtype=np.float64).reshape(-1, 2)
        assigned: Dict[int, Dict] = {}
        for face in faces:
            x1, y1, x2, y2 = face["bbox"][:4]
            cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
            track_id = None
            if live_ids:
                dist = np.sqrt((cx - live_xy[:, 0]) ** 2 + (cy - live_xy[:, 1]) ** 2)
                nearest = int(np.argmin(dist))
                if dist[nearest] < limit and live_ids[nearest] not in assigned:
                    track_id = live_ids[nearest]
            if track_id is None:
                track_id = self.next_track_id
                self.next_track_id += 1
            assigned[track_id] = {"x": cx, "y": cy, "face": face}
        self.active_tracks = {t: dict(entry) for t, entry in assigned.items()}
        return assigned

    def _recognize_face(self, face_data: Dict, track_id: int, timestamp: Optional[str] = None) -> Optional[Dict]:
        self.total_recognition_attempts += 1
        embedding = self.embedder.extract_embedding(face_data["aligned_face"], normalize=True)
        results = self.gallery.search(embedding, top_k=3)
        return self._result_of(results, track_id, face_data, timestamp or datetime.now().isoformat())

    def _settle(self, track_id: int, result: Optional[Dict], aligned_face, original_crop,
                events: List[tuple]) -> None:
        """What ``process_frame`` does with an attempt's result (:357-390)."""
        if result is None:
            return
        if result["recognized"]:
            self.tracker.mark_recognized(track_id, result)
            result["saved_face_path"] = self._save_face_image(aligned_face, track_id, result["student_id"],
                                                              result["name"], result["confidence"], recognized=True,
                                                              original_crop=original_crop)
            events.append(("recognized", result))
            self._print(f"[Frame {self.frame_count}] Recognized: {result['name']} "
                        f"(track_{track_id:04d}, confidence: {result['confidence']:.3f})")
        else:
            self._print(f"[Frame {self.frame_count}] Below threshold: {result['name']} "
                        f"(track_{track_id:04d}, confidence: {result['confidence']:.3f}, "
                        f"threshold: {self.similarity_threshold})")
            if self.tracker.recognition_attempts.get(track_id, 0) >= self.max_recognition_attempts:
                result["saved_face_path"] = self._save_face_image(aligned_face, track_id, result["student_id"],
                                                                  result["name"], result["confidence"],
                                                                  recognized=False)
                events.append(("unrecognized", result))

    def process_frame(self, frame: np.ndarray, timestamp: Optional[str] = None) -> Dict:
        """:320-414 on one BGR frame: detect, assign to tracks, buffer, and on a recognition frame
        embed and search the best buffered face of every unresolved track."""
        self.frame_count += 1
        timestamp = timestamp or datetime.now().isoformat()
        frame_rgb = np.ascontiguousarray(np.asarray(frame)[..., ::-1])
        faces = self.face_processor.process_numpy(frame_rgb, return_all=True)
        for face in faces:
            x1, y1, x2, y2 = map(int, face["bbox"])
            face["original_crop"] = frame_rgb[y1:y2, x1:x2].copy()
        self.total_faces_detected += len(faces)
        tracked_faces = self._simple_track_assignment(faces)
        recognition_events: List[tuple] = []
        for track_id, track_data in tracked_faces.items():
            face = track_data["face"]
            self.tracker.add_frame(track_id, face, timestamp)
            if self.tracker.should_recognize(track_id, self.frame_count):
                best_frame = self.tracker.get_best_frame(track_id)
                if best_frame is not None:
                    result = self._recognize_face(best_frame, track_id, timestamp)
                    self.tracker.increment_attempts(track_id)
                    self._settle(track_id, result, best_frame["aligned_face"], best_frame.get("original_crop"),
                                 recognition_events)
        if recognition_events:
            self._update_attendance(recognition_events)
        return {"frame_count": self.frame_count, "faces_detected": len(faces), "active_tracks": len(tracked_faces),
                "recognition_events": len(recognition_events), "performance": {}}

    def _save_face_image(self, aligned_face: np.ndarray, track_id: int, student_id: str, name: str,
                         confidence: float, recognized: bool, original_crop: np.ndarray = None) -> str:
        """:428-456, written with PIL (the reference converts RGB to BGR for cv2.imwrite: the file
        holds the RGB picture)."""
        from PIL import Image
        output_dir = self.recognized_faces_dir if recognized else self.unrecognized_faces_dir
        if recognized:
            output_dir = os.path.join(output_dir, f"{student_id}_{name.replace(' ', '_')}")
            os.makedirs(output_dir, exist_ok=True)
        timestamp = datetime.now().strftime("%Y%m%d_%H%M%S_%f")
        stem = f"track_{track_id:04d}_{timestamp}_conf{confidence:.3f}"
        filepath_aligned = os.path.join(output_dir, f"{stem}_aligned.jpg")
        Image.fromarray(np.ascontiguousarray(aligned_face, dtype=np.uint8)).save(filepath_aligned, quality=95)
        if original_crop is not None and original_crop.size > 0:
            filepath_original = os.path.join(output_dir, f"{stem}_original.jpg")
            Image.fromarray(np.ascontiguousarray(original_crop, dtype=np.uint8)).save(filepath_original, quality=95)
        return filepath_aligned

    def _rate_statistics(self, seconds: float) -> Dict:
        return {"average_fps": self.frame_count / seconds if seconds > 0 else 0}

    def _rate_summary(self, statistics: Dict) -> str:
        return f"\nAverage FPS: {statistics['average_fps']:.1f}"

    def _finalize_session(self):
        """:632-684: close ``session.json`` (end time, status, duration, the statistics with the frame
        rate) and return it."""
        return self._close_session()

    # -- a recorded clip, or one per camera -----------------------------------------------------
    def process_clip(self, frames, timestamps=None, fps: float = 30.0):
        """One live session per clip.  ``frames``: a uint8 [n,H,W,3] BGR clip (array or tensor), or a
        list of clips for several cameras (one ``fr_live_tracks`` launch and at most
        ``max_recognition_attempts`` embed + match batches for all of them; camera c's session is
        written under ``session_dir/camera_%02d`` and kept in ``self.cameras[c]``).  ``timestamps``:
        per frame ISO strings (for a list of clips, one list per clip); default ``session_start +
        i / fps``.  Returns per clip ``{'frames_processed', 'faces_detected', 'tracks_opened',
        'track_id' (per detection, detection order), 'frame_offsets', 'attempts' (``resolve_attempts``'
        log with the detection's frame as 'frame'), 'events' ([(frame index, type, result), ...]),
        'session_dir'}``.  The session is left unfinalised, as ``process_frame`` leaves it."""
        import torch
        from .face_detection import CameraFaceCapture
        many = isinstance(frames, (list, tuple))
        clips = list(frames) if many else [frames]
        stamps = list(timestamps) if (many and timestamps is not None) else [timestamps] * len(clips)
        if len(stamps) != len(clips):
            raise ValueError("timestamps: one list per clip")
        p = self.face_processor
        device = p.aligner._ops.device
        shim = types.SimpleNamespace(processor=p, skip_frames=1, device=device,
                                     device_chain=getattr(self, "device_chain", False))
        per_clip = []
        for c in clips:  # detect -> align -> blur -> gate, the crops left on the device
            if isinstance(c, torch.Tensor):
                rgb = c.flip(-1)
            else:
                rgb = torch.from_numpy(np.ascontiguousarray(np.asarray(c, dtype=np.uint8)[..., ::-1]))
            per_clip.append(CameraFaceCapture._faces_of_clip(shim, rgb) + (rgb,))
        faces = [f for _picked, per_frame, _crops, _rgb in per_clip for fr in per_frame for f in fr]
        bbox = np.array([np.asarray(f["bbox"]).astype(int)[:4] for f in faces], dtype=np.int64).reshape(-1, 4)
        metrics = np.array([[f["det_score"], f["quality_metrics"].get("blur_score", 0)] for f in faces],
                           dtype=np.float64).reshape(-1, 2)
        if not np.isfinite(metrics).all():
            raise ValueError("non-finite quality metrics (det_score, blur_score)")
        if len(faces) and np.abs(bbox).max() > CAPTURE_COORD_MAX:
            raise NotImplementedError(f"a box coordinate beyond +-{CAPTURE_COORD_MAX}")
        frame_offsets = np.concatenate([[0], np.cumsum([len(fr) for _p, per_frame, _c, _r in per_clip
                                                        for fr in per_frame])]).astype(np.int32)
        clip_offsets = np.concatenate([[0], np.cumsum([len(per_frame) for _p, per_frame, _c, _r in per_clip])]
                                      ).astype(np.int32)
        handle = self.embedder.model
        dev = handle.device
        track_id, _prev, attempt, best, info = (x.cpu().numpy() for x in handle.live_tracks(
            torch.from_numpy(bbox.astype(np.int32)).to(dev), torch.from_numpy(metrics).to(dev), frame_offsets,
            clip_offsets, self.max_distance, self.recognition_interval, self.max_recognition_attempts,
            self._frame_buffer_size))
        det_clip = np.repeat(np.arange(len(clips)), np.diff(frame_offsets[clip_offsets]))
        det_frame = np.repeat(np.arange(len(frame_offsets) - 1), np.diff(frame_offsets))  # global frame index
        crops = torch.cat([c for _p, _f, c, _r in per_clip]) if per_clip else None
        rows = np.array([f["crop_row"] for f in faces], dtype=np.int64)
        base = np.concatenate([[0], np.cumsum([len(c) for _p, _f, c, _r in per_clip])])
        rows = rows + base[det_clip] if len(faces) else rows

        def recognise(dets: List[int]):
            picked = crops[torch.from_numpy(rows[dets]).to(crops.device)].contiguous()
            if tuple(picked.shape[1:3]) != (112, 112):  # face_embedder.py:94-96, on the device
                resized = torch.empty((len(dets), 112, 112, 3), dtype=torch.uint8, device=picked.device)
                handle.resize_crops(picked, resized)
                picked = resized
            return self.gallery.match_resolved(len(dets), 3,
                                               lambda h, k, idx, score: h.embed_match(picked, k, idx, score))

        keys = [(int(c), int(t)) for c, t in zip(det_clip, track_id)]
        log, events = resolve_attempts(keys, attempt, best, recognise, self.similarity_threshold,
                                       self.max_recognition_attempts)
        # the crops the events save, in one copy
        saved = sorted({e["best"] for e in events})
        host = crops[torch.from_numpy(rows[saved]).to(crops.device)].cpu().numpy() if saved else None
        saved_at = {d: i for i, d in enumerate(saved)}
        # the reference's bookkeeping, per clip, in (frame, detection) order
        self.cameras = [self._camera(c) for c in range(len(clips))] if many else [self]
        if not many:
            self._start_session()
        out = []
        for c, cam in enumerate(self.cameras):
            f0, f1 = int(clip_offsets[c]), int(clip_offsets[c + 1])
            d0, d1 = int(frame_offsets[f0]), int(frame_offsets[f1])
            ts = stamps[c]
            if ts is None:
                ts = [(cam.session_start + timedelta(seconds=i / fps)).isoformat() for i in range(f1 - f0)]
            if len(ts) != f1 - f0:
                raise ValueError(f"clip {c}: {len(ts)} timestamps for {f1 - f0} frames")
            rgb = per_clip[c][3]
            tr = cam.tracker
            for d in range(d0, d1):  # first / last seen of every track, as add_frame leaves them
                tid, t = int(track_id[d]), ts[det_frame[d] - f0]
                tr.track_first_seen.setdefault(tid, t)
                tr.track_last_seen[tid] = t
            last_seen = dict(tr.track_last_seen)
            my_log = [e for e in log if d0 <= e["det"] < d1]
            my_events = {e["det"]: e for e in events if d0 <= e["det"] < d1}
            clip_events, frame_events, at_frame = [], [], None
            for e in my_log + [None]:
                f = None if e is None else int(det_frame[e["det"]]) - f0
                if frame_events and f != at_frame:  # the frame's events, once the frame is over
                    cam._update_attendance(frame_events)
                    clip_events += [(at_frame, kind, result) for kind, result in frame_events]
                    frame_events = []
                if e is None:
                    break
                at_frame = f
                tid = e["track"][1]
                cam.frame_count = f + 1
                cam.total_recognition_attempts += 1
                tr.track_last_seen[tid] = ts[f]  # the duration an event reports ends at its frame
                tr.increment_attempts(tid)
                face = faces[e["best"]]
                result = cam._result_of(e["matches"], tid, face, ts[f])
                if e["det"] in my_events:
                    x1, y1, x2, y2 = map(int, face["bbox"])
                    original = rgb[int(det_frame[e["best"]]) - f0, y1:y2, x1:x2].cpu().numpy()
                    cam._settle(tid, result, host[saved_at[e["best"]]], original, frame_events)
                elif result is not None:
                    cam._settle(tid, result, None, None, frame_events)  # below the threshold, attempts left
            tr.track_last_seen.update(last_seen)
            cam.frame_count = f1 - f0
            cam.total_faces_detected = d1 - d0
            cam.next_track_id = int(info[c, 0])
            last = frame_offsets[f1 - 1:f1 + 1] if f1 > f0 else [0, 0]
            cam.active_tracks = {int(track_id[d]): {"x": (bbox[d, 0] + bbox[d, 2]) / 2,
                                                    "y": (bbox[d, 1] + bbox[d, 3]) / 2, "face": faces[d]}
                                 for d in range(int(last[0]), int(last[1]))}
            out.append({"frames_processed": f1 - f0, "faces_detected": d1 - d0, "tracks_opened": int(info[c, 0]),
                        "track_id": track_id[d0:d1].copy(), "frame_offsets": frame_offsets[f0:f1 + 1] - d0,
                        "attempts": [dict(e, det=e["det"] - d0, best=e["best"] - d0, track=e["track"][1],
                                          frame=int(det_frame[e["det"]]) - f0) for e in my_log],
                        "events": clip_events, "session_dir": cam.session_dir})
        self.last_clip_info = info
        return out if many else out[0]
