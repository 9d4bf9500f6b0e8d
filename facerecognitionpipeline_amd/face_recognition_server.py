"""``LiveRecognitionTracker`` / ``FaceRecognitionServer`` / ``create_app`` — the reference's attendance
server (face_recognition_server.py:23-1106): requests from a camera client in, ``attendance.json`` +
``session.json``, the saved face crops and the snapshots of a session folder out.

The server's tracker is not the live loop's (face_recognition_live.py): it has no every-N-frames gate
(``recognition_interval`` is stored and never read), it gates on the detection score of the best
buffered face, it has a wall-clock retry cooldown that resets the attempts and empties the ring, and
its track ids come from outside: the client's in ``process_faces``, a fresh one per face in
``process_full_frame``.  What it shares with the live loop's is in attendance_session.py
(``TrackRecords``), as is the shared part of the two session classes (``AttendanceSession``) and of the
two resolvers.  The two flows also share that an attempt depends on earlier recognition results only
through "this track is already recognised"; everything else follows from the detections and the clock.  So a recorded log replays exactly: ``fr_server_tracks`` (contract:
``server_tracks_host``) decides every track's attempts in one launch, ``resolve_server_attempts``
embeds and matches them an ordinal at a time, and ``process_requests`` / ``process_frames`` replay the
bookkeeping in request order.

Notes on parity:

* The clock.  The reference reads ``time.time()`` twice per ``should_recognize``; here the tracker's
  ``clock`` (injectable, default ``time.time``) is read once per request and that value serves every
  face of it.
* ``process_faces`` omits the reference's ``self.tracker.cleanup_stale_tracks(...)`` call, which
  raises ``AttributeError`` as committed (the method sits on the server class and reads an attribute
  the server does not have).
* PNGs are written and decoded with PIL; the bytes against ``cv2.imencode`` are UNPINNED, as for the
  JPEGs elsewhere.  ``original_crop`` is cut only for a face whose event saves it, a recognised one
  (the reference cuts and encodes one for every face and saves the same ones); one over 600 px is
  resized with PIL's Lanczos filter, UNPINNED against ``cv2.INTER_LANCZOS4``.
* ``timestamp`` of a result is the request's (the reference calls ``datetime.now()`` again inside
  ``_recognize_face``).  ``process_faces(..., timestamp=...)`` takes an ISO string; the default is the
  wall clock.
* All due faces of a request go through one ``fr_embed_match``.  A track id that occurs twice in one
  request is handled in a second round, after the first occurrence's result is known, so the outcome
  is the one of the face-by-face loop.
* ``performance`` is ``{}``, the reference's value without a monitor: the performance monitors are out
  of scope (``enable_performance_monitoring`` / ``enable_gpu_monitoring`` are accepted and stored;
  ``perf_monitor`` is None).  ``use_gpu`` is accepted and not read: there is no CPU path.
* Ring entries made by the batched calls hold the face's ``aligned_face`` array; its PNG is encoded
  only when the face is saved.
"""
from __future__ import annotations

import argparse
import base64
import io
import math
import os
import time
from datetime import datetime
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .attendance_session import AttendanceSession, TrackRecords, _resolve, selection_key

# include/frhip.h FR_SERVER_*
SERVER_MAX_ATTEMPTS = 16
SERVER_MAX_BUFFER = 64
SERVER_GATED, SERVER_ATTEMPT, SERVER_COOLDOWN, SERVER_COOLDOWN_SET, SERVER_RESET = range(5)
SERVER_ERR_VALUE = 1
SERVER_ERR_ORDER = 2
DET_GATE = 0.6  # should_recognize's `best.get('det_score', 0) > 0.6`


def _check_settings(max_attempts, buffer_size, retry_cooldown, det_gate=DET_GATE) -> None:
    if not 1 <= int(max_attempts) <= SERVER_MAX_ATTEMPTS:
        raise ValueError(f"max_attempts must be in [1, {SERVER_MAX_ATTEMPTS}]")
    if not 1 <= int(buffer_size) <= SERVER_MAX_BUFFER:
        raise ValueError(f"buffer_size must be in [1, {SERVER_MAX_BUFFER}]")
    if not (math.isfinite(retry_cooldown) and retry_cooldown >= 0):
        raise ValueError("retry_cooldown must be finite and >= 0")
    if not math.isfinite(det_gate):
        raise ValueError("det_gate must be finite")


def group_by_track(track_ids) -> tuple:
    """(order int32 [n], track_offsets int32 [T+1], the T distinct ids in ascending order): the
    detections grouped by track id with a stable sort, so arrival order holds within a track."""
    ids = np.asarray(track_ids).reshape(-1)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    keys, counts = np.unique(ids, return_counts=True)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), keys


def server_tracks_host(metrics, clock, order, track_offsets, max_attempts: int = 3, buffer_size: int = 10,
                       retry_cooldown: float = 10.0, det_gate: float = DET_GATE, trace: Optional[set] = None):
    """What ``fr_server_tracks`` computes, in plain Python: ``metrics`` float64 [n,2] (det_score,
    blur_score), ``clock`` float64 [n] (seconds; a request's clock repeated for its faces), track t =
    detections ``order[track_offsets[t]:track_offsets[t+1]]`` in arrival order.  Returns ``(attempt
    int32 [n], best int32 [n], state int32 [n], track_info int32 [T,4] = attempts, cooldowns set,
    resets, error)``.

    ``trace`` (a set) collects the names of the situations the log went through: the tests use it to
    show that a fixture reaches them."""
    _check_settings(max_attempts, buffer_size, retry_cooldown, det_gate)
    metrics = np.asarray(metrics, dtype=np.float64).reshape(-1, 2)
    clock = np.asarray(clock, dtype=np.float64).reshape(-1)
    order = [int(v) for v in np.asarray(order).reshape(-1)]
    off = [int(v) for v in np.asarray(track_offsets).reshape(-1)]
    n = metrics.shape[0]
    if clock.shape[0] != n:
        raise ValueError("clock must have one entry per row of metrics")
    if len(off) < 1 or off[0] != 0 or off[-1] != len(order) or any(b < a for a, b in zip(off[:-1], off[1:])):
        raise ValueError("track_offsets must rise from 0 to the number of entries of order")
    ev = trace.add if trace is not None else (lambda name: None)
    max_attempts, buffer_size = int(max_attempts), int(buffer_size)
    retry_cooldown, det_gate = float(retry_cooldown), float(det_gate)
    attempt, best = (np.full(n, -1, np.int32) for _ in range(2))
    state = np.zeros(n, np.int32)
    info = np.zeros((len(off) - 1, 4), np.int32)
    key = [selection_key(float(m[0]), float(m[1])) for m in metrics]
    if len(off) > 1 and all(b - a == 1 for a, b in zip(off[:-1], off[1:])):
        ev("fresh_id_per_face")
    if buffer_size == 1:
        ev("buffer_size_one")
    for t in range(len(off) - 1):
        mine = order[off[t]:off[t + 1]]
        error = 0
        if any(not 0 <= d < n for d in mine):
            error |= SERVER_ERR_ORDER
        if any(0 <= d < n and not (np.isfinite(metrics[d]).all() and np.isfinite(clock[d])) for d in mine):
            error |= SERVER_ERR_VALUE
        if error:
            for d in mine:
                if 0 <= d < n:
                    attempt[d], best[d], state[d] = -1, -1, SERVER_GATED
            info[t] = [0, 0, 0, error]
            continue
        attempts = made = cooldowns = resets = run_start = 0
        deadline = None
        dropped = None  # the appearance a reset cleared, until the next selection
        for j, d in enumerate(mine):
            now = float(clock[d])
            if metrics[d, 1] == 100.0:
                ev("blur_exactly_100")
            if metrics[d, 1] > 100.0:
                ev("blur_over_100")
            if deadline is not None:
                if now < deadline:
                    state[d] = SERVER_COOLDOWN
                    ev("silent_in_cooldown")
                    continue
                if now == deadline:
                    ev("exactly_at_deadline")
                deadline, attempts, run_start, dropped = None, 0, j + 1, j
                resets += 1
                state[d] = SERVER_RESET
                continue
            if attempts >= max_attempts:
                deadline = now + retry_cooldown
                cooldowns += 1
                state[d] = SERVER_COOLDOWN_SET
                ev("cooldown_set_on_next_appearance")
                if retry_cooldown == 0.0:
                    ev("retry_cooldown_zero")
                continue
            window = mine[max(run_start, j - buffer_size + 1):j + 1]  # oldest first, as the deque
            pick = max(window, key=lambda i: key[i])  # the first of equal keys: the oldest
            det = float(metrics[pick, 0])
            if trace is not None:
                if sum(key[i] == key[pick] for i in window) > 1:
                    ev("equal_keys_oldest_wins")
                older = mine[run_start:max(run_start, j - buffer_size + 1)]
                if older and max(key[i] for i in older) > key[pick]:
                    ev("best_evicted_from_ring")
                if dropped is not None and j - dropped < buffer_size and key[mine[dropped]] > key[pick]:
                    ev("reset_drops_current_face")
                if det == det_gate:
                    ev("det_exactly_at_gate")
                if det == np.nextafter(det_gate, np.inf):
                    ev("det_next_double_above_gate")
                if det <= det_gate and pick != d and metrics[d, 0] > det_gate:
                    ev("gated_best_blocks_newer")
            dropped = None
            if det > det_gate:
                attempt[d], best[d], state[d] = made, pick, SERVER_ATTEMPT
                made += 1
                attempts += 1
            else:
                state[d] = SERVER_GATED
        if deadline is not None:
            ev("left_in_cooldown")
        info[t] = [made, cooldowns, resets, 0]
    return attempt, best, state, info


def resolve_server_attempts(track_key: Sequence, attempt, best, recognise: Callable[[List[int]], List[List]],
                            similarity_threshold: float, max_attempts: int, trace: Optional[set] = None):
    """The attempts the reference makes, out of ``fr_server_tracks``' speculative candidates.
    ``track_key[d]`` names detection d's track (any hashable), ``attempt`` / ``best`` are the kernel's
    arrays.  For ordinal k = 0, 1, ... the ``best`` detections of the ordinal-k candidates whose track
    is not yet recognised go through one ``recognise(list of detection indices)`` call, which returns
    per entry the ``gallery.search(top_k=3)`` list ``[(student_id, name, score), ...]``.  A success
    drops the track's later candidates; a failure with ``k % max_attempts == max_attempts - 1`` is an
    ``unrecognized`` event (one per cooldown cycle).  Returns ``(log, events)``: ``log`` = the attempts
    made, ``{'det', 'track', 'attempt', 'best', 'matches'}``; ``events`` = the same with ``'type'``
    ('recognized' | 'unrecognized'); both in detection order, which is request order, then face order.
    An empty ``matches`` (empty gallery) counts as an attempt and yields nothing, as in the reference."""
    ordinals = np.unique(np.asarray(attempt).reshape(-1))
    return _resolve([int(k) for k in ordinals if k >= 0], track_key, attempt, best, recognise, similarity_threshold,
                    max_attempts, trace)


class LiveRecognitionTracker(TrackRecords):
    """face_recognition_server.py:23-124: the records of every track id ever seen (the attempts are
    those of the current cycle), and the deadline of its retry cooldown.  ``recognition_interval`` is
    stored; ``should_recognize`` does not read it.  ``clock`` returns seconds (default ``time.time``);
    every method that needs the time also takes it as ``now``."""

    def __init__(self, recognition_interval=30, max_attempts=3, buffer_size=10, retry_cooldown=10.0,
                 clock: Callable[[], float] = time.time):
        super().__init__(recognition_interval, max_attempts, buffer_size)
        self.track_last_attempt: Dict = {}
        self.client_tracks: Dict = {}          # never written (the reference's writer is commented out)
        self.track_cooldowns: Dict = {}        # track id -> deadline in clock seconds
        self.retry_cooldown = retry_cooldown
        self.clock = clock

    def should_recognize(self, track_id, frame_count: int, now: Optional[float] = None) -> bool:
        if track_id in self.recognized_tracks:
            return False
        now = self.clock() if now is None else now
        if self.is_track_in_cooldown(track_id, now):
            return False
        if self.recognition_attempts.get(track_id, 0) >= self.max_attempts:
            self.set_track_cooldown(track_id, self.retry_cooldown, now)
            return False
        face = self.get_best_frame(track_id)
        return face is not None and face.get("det_score", 0) > DET_GATE

    def increment_attempts(self, track_id):
        super().increment_attempts(track_id)
        self.track_last_attempt[track_id] = datetime.now().isoformat()

    def is_track_in_cooldown(self, track_id, now: Optional[float] = None) -> bool:
        """True before the deadline.  At or past it the cooldown ends: the attempts go to 0 and the
        ring is emptied (the face just added included)."""
        deadline = self.track_cooldowns.get(track_id)
        if deadline is None:
            return False
        now = self.clock() if now is None else now
        if now < deadline:
            return True
        self.end_cooldown(track_id)
        return False

    def end_cooldown(self, track_id):
        del self.track_cooldowns[track_id]
        self.recognition_attempts[track_id] = 0
        ring = self.track_frame_buffers.get(track_id)
        if ring is not None:
            ring.clear()

    def set_track_cooldown(self, track_id, cooldown_seconds: float = 3.0, now: Optional[float] = None):
        now = self.clock() if now is None else now
        self.track_cooldowns[track_id] = now + cooldown_seconds


def encode_png(image: np.ndarray) -> str:
    """An RGB (or gray) uint8 image as the base64 text of its PNG (compression 3, as the reference asks
    of cv2)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(image, dtype=np.uint8)).save(buf, format="PNG", compress_level=3)
    return base64.b64encode(buf.getvalue()).decode("utf-8")


def decode_image(data: bytes) -> np.ndarray:
    """Encoded image bytes (PNG, JPEG, ...) as an RGB uint8 array (``cv2.imdecode(IMREAD_COLOR)`` +
    ``BGR2RGB``)."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


class FaceRecognitionServer(AttendanceSession):
    """face_recognition_server.py:126-840.  ``processor`` (a ``FaceProcessor``, or anything with its
    ``process_numpy``; ``process_frames`` also needs ``process_images``), ``embedder`` and ``gallery``
    default to the reference's settings (:155-200).  With a ``FaceEmbedder`` and a ``GalleryManager``
    the due faces of a request are embedded and matched in one ``fr_embed_match``; stand-ins that only
    have ``extract_embedding`` / ``search`` are asked face by face."""

    SUMMARY_INDENT = "  "

    def __init__(self, gallery_path="gallery/students.pkl", similarity_threshold=0.5, output_dir="sessions",
                 session_name=None, require_session_name=False, recognition_interval=30, max_recognition_attempts=3,
                 frame_buffer_size=10, enable_performance_monitoring=True, enable_gpu_monitoring=True, use_gpu=True,
                 model_type="adaface", architecture="ir_101", model_path=None, device=None, processor=None,
                 embedder=None, gallery=None, retry_cooldown: float = 10.0, clock: Callable[[], float] = time.time,
                 verbose: bool = True):
        self.verbose = verbose
        self._print("\n" + "=" * 70)
        self._print("INITIALIZING FACE RECOGNITION SERVER")
        self._print("=" * 70)
        self.similarity_threshold = similarity_threshold
        self.recognition_interval = recognition_interval
        self.max_recognition_attempts = max_recognition_attempts
        self.output_dir = output_dir
        self.require_session_name = require_session_name
        self.enable_performance_monitoring = enable_performance_monitoring
        self.enable_gpu_monitoring = enable_gpu_monitoring
        self.frame_buffer_size = frame_buffer_size
        self.retry_cooldown = retry_cooldown  # _create_session builds the tracker without one: 10.0
        self.clock = clock
        _check_settings(max_recognition_attempts, frame_buffer_size, retry_cooldown)
        self._load_embedder(embedder, architecture, model_path, model_type, device)
        self._load_processor(processor, device)
        self.high_quality_crop_size = 600
        self.max_tracking_distance = 100
        self.next_track_id = 0
        self._load_gallery(gallery, gallery_path)
        self.session_name = None
        self.session_dir = None
        self.session_start = None
        self.recognized_faces_dir = None
        self.unrecognized_faces_dir = None
        self.snapshots_dir = None
        self.perf_monitor = None
        self.tracker: Optional[LiveRecognitionTracker] = None
        self.trace: Optional[set] = None  # the tests' record of the situations the requests met
        self.frame_count = 0
        self.total_faces_detected = 0
        self.total_recognition_attempts = 0
        if session_name:
            self._create_session(session_name)
        else:
            self._print("\n" + "=" * 70)
            self._print("Server ready!\nWaiting for client to initialize session...")
            self._print(f"Recognition interval: every {recognition_interval} frames")
            self._print(f"Similarity threshold: {similarity_threshold}")
            self._print("=" * 70 + "\n")

    # -- the session (:230-262) ----------------------------------------------------------------
    def _create_session(self, session_name: str):
        self.session_name = session_name
        self.session_dir = os.path.join(self.output_dir, self.session_name)
        self._open_session(LiveRecognitionTracker(recognition_interval=self.recognition_interval,
                                                  max_attempts=self.max_recognition_attempts,
                                                  buffer_size=self.frame_buffer_size,
                                                  retry_cooldown=self.retry_cooldown, clock=self.clock))
        self.snapshots_dir = os.path.join(self.session_dir, "snapshots")
        os.makedirs(self.snapshots_dir, exist_ok=True)
        self._print("\n" + "=" * 70)
        self._print(f"Session created: {self.session_name}\nOutput: {self.session_dir}")
        self._print("=" * 70 + "\n")

    # -- recognition (:314-347) ------------------------------------------------------------------
    @staticmethod
    def _aligned_of(face_data: Dict) -> np.ndarray:
        face = face_data.get("aligned_face")
        if face is None:
            face = decode_image(base64.b64decode(face_data["aligned_face_base64"]))
        return np.asarray(face)

    def _search_faces(self, faces_data: List[Dict]) -> List[List]:
        """``gallery.search(embedding, top_k=3)`` of every face: one ``fr_embed_match`` for all of them
        on the device models, face by face on stand-ins."""
        if not faces_data:
            return []
        crops = [self._aligned_of(f) for f in faces_data]
        if hasattr(self.embedder, "to_device_crops") and hasattr(self.gallery, "match_resolved"):
            rgb = self.embedder.to_device_crops(crops)
            return self.gallery.match_resolved(len(crops), 3,
                                               lambda h, k, idx, score: h.embed_match(rgb, k, idx, score))
        return [self.gallery.search(self.embedder.extract_embedding(c, normalize=True), top_k=3) for c in crops]

    def _recognize_face(self, face_data: Dict, track_id, timestamp: Optional[str] = None) -> Optional[Dict]:
        self.total_recognition_attempts += 1
        return self._result_of(self._search_faces([face_data])[0], track_id, face_data,
                               timestamp or datetime.now().isoformat())

    def _settle(self, track_id, result: Optional[Dict], best_frame: Dict, events: List[tuple]) -> None:
        """What the request loops do with an attempt's result (:380-413, :649-678)."""
        if result is None:
            return
        if result["recognized"]:
            self.tracker.mark_recognized(track_id, result)
            kind = "recognized"
            self._print(f"[Frame {self.frame_count}] Recognized: {result['name']} "
                        f"(track_{track_id:04d}, confidence: {result['confidence']:.3f})")
        else:
            self._print(f"[Frame {self.frame_count}] Below threshold: {result['name']} "
                        f"(track_{track_id:04d}, confidence: {result['confidence']:.3f}, "
                        f"threshold: {self.similarity_threshold})")
            if self.tracker.recognition_attempts.get(track_id, 0) < self.max_recognition_attempts:
                return
            kind = "unrecognized"
        aligned = best_frame.get("aligned_face_base64") or encode_png(best_frame["aligned_face"])
        original = None  # saved beside a recognised face only, as in the reference
        if kind == "recognized":
            original = best_frame.get("original_crop_base64")
            if original is None and best_frame.get("_frame") is not None:
                crop = self._high_quality_crop(best_frame["_frame"], best_frame["bbox"])
                original = encode_png(crop) if crop.size > 0 else None
        result["saved_face_path"] = self._save_face_image(aligned, track_id, result["student_id"], result["name"],
                                                          result["confidence"], recognized=kind == "recognized",
                                                          original_crop_base64=original)
        events.append((kind, result))

    def _run_request(self, faces_data: List[Dict], timestamp: str, now: float) -> List[tuple]:
        """The loop of :368-413 over the faces of one request, the due faces embedded and matched
        together.  A face whose track already has an attempt pending in this request waits for a
        further round, so it sees that attempt's outcome as in the face-by-face loop."""
        tr = self.tracker
        found: Dict[int, tuple] = {}
        pending = list(enumerate(faces_data))
        if len({f["track_id"] for f in faces_data}) < len(faces_data):
            self._note("track_twice_in_request")
        while pending:
            due, later, busy = [], [], set()
            for i, face_data in pending:
                track_id = face_data["track_id"]
                if track_id in busy:
                    later.append((i, face_data))
                    continue
                tr.add_frame(track_id, face_data, timestamp)
                if tr.should_recognize(track_id, self.frame_count, now):
                    best_frame = tr.get_best_frame(track_id)
                    if best_frame is not None:
                        due.append((i, track_id, best_frame))
                        busy.add(track_id)
            self.total_recognition_attempts += len(due)
            for (i, track_id, best_frame), matches in zip(due, self._search_faces([b for _i, _t, b in due])):
                tr.increment_attempts(track_id)
                one: List[tuple] = []
                self._settle(track_id, self._result_of(matches, track_id, best_frame, timestamp), best_frame, one)
                if one:
                    found[i] = one[0]
            pending = later
        events = [found[i] for i in sorted(found)]
        # a further round resolved tracks out of face order: put this request's entries back into it
        mine = [r["track_id"] for kind, r in events if kind == "recognized"]
        for track_id in mine:
            tr.recognized_tracks[track_id] = tr.recognized_tracks.pop(track_id)
        return events

    def _tracker_summary(self) -> Dict:
        tr = self.tracker
        return {
            "recognized_tracks": {str(k): v for k, v in tr.recognized_tracks.items()},
            "recognition_attempts": {str(k): v for k, v in tr.recognition_attempts.items()},
            "failed_tracks": {str(k): True for k, v in tr.recognition_attempts.items()
                              if v >= self.max_recognition_attempts and k not in tr.recognized_tracks},
        }

    def _faces_result(self, n_faces: int, events: List[tuple]) -> Dict:
        return {"frame_count": self.frame_count, "faces_processed": n_faces, "recognition_events": len(events),
                **self._tracker_summary(),
                "tracks_in_cooldown": {str(k): True for k in self.tracker.track_cooldowns},
                "performance": {}}

    def _frame_result(self, faces_data: List[Dict], events: List[tuple]) -> Dict:
        return {
            "frame_count": self.frame_count,
            "faces_detected": len(faces_data),
            "active_tracks": len(faces_data),
            "tracks": [{"track_id": f["track_id"], "bbox": f["bbox"], "det_score": f["det_score"]}
                       for f in faces_data],
            **self._tracker_summary(),
            "newly_recognized": {str(r["track_id"]): {k: r[k] for k in ("student_id", "name", "confidence",
                                                                         "timestamp")}
                                 for kind, r in events if kind == "recognized"},
            "newly_failed": [str(r["track_id"]) for kind, r in events if kind == "unrecognized"],
            "performance": {},
        }

    def process_faces(self, faces_data: List[Dict], frame_count: int, timestamp: Optional[str] = None) -> Dict:
        """:349-444: the faces a client detected, aligned and tracked (``track_id``, ``det_score``,
        ``quality_metrics``, ``aligned_face_base64``, optionally ``original_crop_base64``).  The
        reference's ``cleanup_stale_tracks`` call, which raises ``AttributeError`` as committed, is
        omitted."""
        self.frame_count = frame_count
        timestamp = timestamp or datetime.now().isoformat()
        now = self.tracker.clock()
        if not faces_data:
            self._note("empty_request")
        self.total_faces_detected += len(faces_data)
        events = self._run_request(faces_data, timestamp, now)
        if events:
            self._update_attendance(events)
        return self._faces_result(len(faces_data), events)

    def _save_face_image(self, aligned_face_base64: str, track_id, student_id: str, name: str, confidence: float,
                         recognized: bool, original_crop_base64: str = None) -> str:
        output_dir = self.recognized_faces_dir if recognized else self.unrecognized_faces_dir
        if recognized:
            output_dir = os.path.join(output_dir, f"{student_id}_{name.replace(' ', '_')}")
            os.makedirs(output_dir, exist_ok=True)
        stamp = datetime.now().strftime("%Y%m%d_%H%M%S_%f")
        stem = os.path.join(output_dir, f"track_{track_id:04d}_{stamp}_conf{confidence:.3f}")
        with open(stem + "_aligned.png", "wb") as f:
            f.write(base64.b64decode(aligned_face_base64))
        if original_crop_base64:
            with open(stem + "_original.png", "wb") as f:
                f.write(base64.b64decode(original_crop_base64))
        return stem + "_aligned.png"

    def save_snapshot(self, snapshot_base64: str, frame_count: int, timestamp: str) -> str:
        filepath = os.path.join(self.snapshots_dir, f"snapshot_frame_{frame_count:06d}_{timestamp}.png")
        with open(filepath, "wb") as f:
            f.write(base64.b64decode(snapshot_base64))
        return filepath

    def finalize_session(self, client_report: Optional[Dict] = None):
        """:538-584: close ``session.json`` (end time, status, duration, the statistics) and return it
        (the reference returns nothing).  ``client_report`` went to the performance monitor and is
        ignored."""
        return self._close_session()

    # -- whole frames (:586-823) -------------------------------------------------------------------
    def _high_quality_crop(self, frame_rgb: np.ndarray, bbox) -> np.ndarray:
        """:599-616: the box widened by 30 % of its longer side, clipped to the frame, and brought down
        to ``high_quality_crop_size`` on its longer side (PIL Lanczos) when it is larger."""
        x1, y1, x2, y2 = map(int, bbox[:4])
        margin = int(max(x2 - x1, y2 - y1) * 0.3)
        crop = frame_rgb[max(0, y1 - margin):min(frame_rgb.shape[0], y2 + margin),
                         max(0, x1 - margin):min(frame_rgb.shape[1], x2 + margin)].copy()
        limit = self.high_quality_crop_size
        if crop.shape[0] > limit or crop.shape[1] > limit:
            from PIL import Image
            scale = limit / max(crop.shape[0], crop.shape[1])
            size = (int(crop.shape[1] * scale), int(crop.shape[0] * scale))
            crop = np.asarray(Image.fromarray(crop).resize(size, Image.LANCZOS))
        return crop

    def _simple_track_assignment(self, faces: List[Dict], timestamp: str) -> Dict:
        """:741-794 as it runs: ``tracker.client_tracks`` is never written, so no face ever finds a
        track and every face of every frame opens the next id, in face order."""
        assigned = {}
        for face in faces:
            x1, y1, x2, y2 = face["bbox"][:4]
            assigned[self.next_track_id] = {"x": (x1 + x2) / 2, "y": (y1 + y2) / 2, "face": face}
            self.next_track_id += 1
        return assigned

    def _prepare_face_data(self, face: Dict, track_id: int, timestamp: str, encode: bool = True) -> Dict:
        """:796-823.  The aligned face also stays in the dict as an array (``aligned_face``), which
        saves the decode on the way to the embedder; ``encode=False`` (the batched calls) leaves the
        PNG to the moment the face is saved."""
        metrics = {k: float(v) if isinstance(v, (np.integer, np.floating)) else v
                   for k, v in face.get("quality_metrics", {}).items()}
        face_data = {"track_id": int(track_id), "bbox": [float(x) for x in face["bbox"]],
                     "det_score": float(face["det_score"]), "quality_metrics": metrics,
                     "aligned_face": face["aligned_face"], "timestamp": timestamp}
        if encode:
            face_data["aligned_face_base64"] = encode_png(face["aligned_face"])
        if "original_crop" in face and face["original_crop"].size > 0:
            face_data["original_crop_base64"] = encode_png(face["original_crop"])
        return face_data

    def process_full_frame(self, frame_rgb: np.ndarray, frame_count: int, timestamp: str) -> Dict:
        """:586-739 on one RGB frame: detect, give every face a fresh id, buffer, embed and search the
        faces that are due."""
        self.frame_count = frame_count
        now = self.tracker.clock()
        faces = self.face_processor.process_numpy(frame_rgb, return_all=True)
        tracked = self._simple_track_assignment(faces, timestamp)
        faces_data = [self._prepare_face_data(data["face"], track_id, timestamp) for track_id, data in tracked.items()]
        for face_data in faces_data:
            face_data["_frame"] = frame_rgb  # for the crop of a face that is recognised in this request
        try:
            events = self._run_request(faces_data, timestamp, now)
        finally:
            for face_data in faces_data:
                del face_data["_frame"]
        if events:
            self._update_attendance(events)
        return self._frame_result(faces_data, events)

    # -- recorded logs -----------------------------------------------------------------------------
    def _launch(self, metrics: np.ndarray, clock: np.ndarray, order: np.ndarray, offsets: np.ndarray):
        import torch
        handle = self.embedder.model
        dev = handle.device
        out = handle.server_tracks(torch.from_numpy(np.ascontiguousarray(metrics, np.float64)).to(dev),
                                   torch.from_numpy(np.ascontiguousarray(clock, np.float64)).to(dev),
                                   torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(dev), offsets,
                                   self.max_recognition_attempts, self.frame_buffer_size, self.retry_cooldown,
                                   DET_GATE)
        return tuple(x.cpu().numpy() for x in out)

    def _replay(self, per_request: List[List[Dict]], frame_counts, timestamps, clocks, whole_frames: bool):
        """Decide every track of the log with one ``fr_server_tracks`` launch, embed and match the
        attempts an ordinal at a time, then do the reference's bookkeeping in request order."""
        flat = [f for faces in per_request for f in faces]
        request_of = np.repeat(np.arange(len(per_request)), [len(faces) for faces in per_request])
        metrics = np.array([[f["det_score"], f["quality_metrics"].get("blur_score", 0)] for f in flat],
                           dtype=np.float64).reshape(-1, 2)
        if not np.isfinite(metrics).all():
            raise ValueError("non-finite quality metrics (det_score, blur_score)")
        clock = np.asarray(clocks, dtype=np.float64).reshape(-1)
        if clock.shape[0] != len(per_request) or not np.isfinite(clock).all():
            raise ValueError("clocks: one finite value per request")
        ids = [f["track_id"] for f in flat]
        dense = {k: i for i, k in enumerate(dict.fromkeys(ids))}  # any hashable id -> a dense int
        order, offsets, _keys = group_by_track(np.array([dense[k] for k in ids], dtype=np.int64))
        attempt, best, state, info = self._launch(metrics, clock[request_of], order, offsets)
        log, _events = resolve_server_attempts(ids, attempt, best, lambda dets: self._search_faces(
            [flat[d] for d in dets]), self.similarity_threshold, self.max_recognition_attempts)
        made = {e["det"]: e for e in log}
        tr = self.tracker
        results, d = [], 0
        for r, faces in enumerate(per_request):
            self.frame_count = frame_counts[r]
            now, timestamp = float(clock[r]), timestamps[r]
            if not faces:
                self._note("empty_request")
            if len({f["track_id"] for f in faces}) < len(faces):
                self._note("track_twice_in_request")
            if not whole_frames:
                self.total_faces_detected += len(faces)
            events: List[tuple] = []
            for face_data in faces:
                track_id = face_data["track_id"]
                tr.add_frame(track_id, face_data, timestamp)
                if track_id not in tr.recognized_tracks:  # a resolved track is left as it is
                    if state[d] == SERVER_RESET:
                        tr.end_cooldown(track_id)
                    elif state[d] == SERVER_COOLDOWN_SET:
                        tr.set_track_cooldown(track_id, self.retry_cooldown, now)
                    elif state[d] == SERVER_ATTEMPT:
                        e = made[d]
                        best_frame = flat[e["best"]]
                        self.total_recognition_attempts += 1
                        tr.increment_attempts(track_id)
                        self._settle(track_id, self._result_of(e["matches"], track_id, best_frame, timestamp),
                                     best_frame, events)
                d += 1
            if events:
                self._update_attendance(events)
            results.append(self._frame_result(faces, events) if whole_frames else self._faces_result(len(faces), events))
        self.last_track_info = info
        return results

    def process_requests(self, requests: Sequence, clocks: Sequence[float], timestamps: Optional[Sequence[str]] = None):
        """A recorded ``process_faces`` log in one call.  ``requests``: per request ``{'faces': [...],
        'frame_count': n}`` (the body the client posts) or ``(faces, frame_count)``; ``clocks``: the
        tracker clock of every request, in seconds; ``timestamps``: their ISO strings (default: the
        wall clock now).  The client ids are made dense on the host with a stable sort, every track is
        decided by one ``fr_server_tracks`` launch, and the attempts go through ``fr_embed_match`` an
        ordinal at a time.  Returns the result dict of every request; tracker, statistics,
        ``attendance.json`` and ``session.json`` end as the ``process_faces`` loop leaves them.  The
        log is a whole session: the call refuses a tracker that has already seen a face."""
        if self.tracker.track_first_seen:
            raise RuntimeError("process_requests replays a whole session: the tracker has already seen faces")
        pairs = [(r["faces"], r.get("frame_count", 0)) if isinstance(r, dict) else (r[0], r[1]) for r in requests]
        if timestamps is None:
            timestamps = [datetime.now().isoformat()] * len(pairs)
        if len(timestamps) != len(pairs):
            raise ValueError("timestamps: one per request")
        return self._replay([list(f) for f, _c in pairs], [c for _f, c in pairs], list(timestamps), clocks, False)

    def process_frames(self, frames: Sequence, frame_counts: Sequence[int], timestamps: Sequence[str],
                       clocks: Sequence[float]):
        """A recorded ``process_full_frame`` log in one call: RGB frames of any sizes through
        ``FaceProcessor.process_images``, a fresh id per face, one ``fr_server_tracks`` launch and one
        embed + match batch for the whole list.  Returns the result dict of every frame; everything
        else ends as the ``process_full_frame`` loop leaves it."""
        if not len(frames) == len(frame_counts) == len(timestamps) == len(clocks):
            raise ValueError("frames, frame_counts, timestamps and clocks: one entry per frame")
        per_frame = self.face_processor.process_images(list(frames), return_all=True)
        per_request = []
        for frame, faces, timestamp in zip(frames, per_frame, timestamps):
            tracked = self._simple_track_assignment(faces, timestamp)
            faces_data = [self._prepare_face_data(data["face"], track_id, timestamp, encode=False)
                          for track_id, data in tracked.items()]
            for face_data in faces_data:
                face_data["_frame"] = np.asarray(frame)
            per_request.append(faces_data)
        try:
            return self._replay(per_request, list(frame_counts), list(timestamps), clocks, True)
        finally:
            for faces_data in per_request:
                for face_data in faces_data:
                    del face_data["_frame"]


def create_app(server: FaceRecognitionServer, debug: bool = False):
    """The reference's Flask routes (:842-969) around ``server``: ``/health``, ``/init_session``,
    ``/process_frame``, ``/save_snapshot``, ``/finalize`` and the ``/process_faces`` it keeps commented
    out.  A failure answers 500 with ``error`` and ``error_type``; ``traceback`` is added only with
    ``debug=True``."""
    from flask import Flask, jsonify, request
    app = Flask(__name__)

    def guarded(needs_session: Optional[str]):
        def wrap(fn):
            def view():
                if needs_session and server.session_name is None:
                    return jsonify({"error": needs_session}), 400
                try:
                    return fn(request.get_json(silent=True) or {})
                except Exception as e:  # the route's own answer, as the reference's
                    details = {"error": str(e), "error_type": type(e).__name__}
                    if debug:
                        import traceback
                        details["traceback"] = traceback.format_exc()
                    return jsonify(details), 500
            view.__name__ = fn.__name__
            return view
        return wrap

    no_session = "No active session. Call /init_session first"

    @app.route("/health", methods=["GET"])
    def health():
        return jsonify({"status": "ok", "session": server.session_name})

    @app.route("/init_session", methods=["POST"])
    @guarded(None)
    def init_session(data):
        session_name = data.get("session_name")
        if not session_name:
            return jsonify({"error": "session_name is required"}), 400
        server._create_session(session_name)
        return jsonify({"status": "session_initialized", "session_name": session_name,
                        "session_dir": server.session_dir})

    @app.route("/process_frame", methods=["POST"])
    @guarded(no_session)
    def process_frame(data):
        frame_rgb = decode_image(base64.b64decode(data.get("frame")))
        return jsonify(server.process_full_frame(frame_rgb, data.get("frame_count", 0),
                                                 data.get("timestamp", datetime.now().isoformat())))

    @app.route("/process_faces", methods=["POST"])
    @guarded(no_session)
    def process_faces(data):
        return jsonify(server.process_faces(data.get("faces", []), data.get("frame_count", 0)))

    @app.route("/save_snapshot", methods=["POST"])
    @guarded(no_session)
    def save_snapshot(data):
        path = server.save_snapshot(data.get("snapshot"), data.get("frame_count", 0),
                                    data.get("timestamp", datetime.now().strftime("%Y%m%d_%H%M%S")))
        return jsonify({"saved": True, "path": path})

    @app.route("/finalize", methods=["POST"])
    @guarded("No active session")
    def finalize(data):
        server.finalize_session(client_report=data.get("client_performance_report"))
        return jsonify({"status": "finalized"})

    return app


def main(argv: Optional[Sequence[str]] = None):
    p = argparse.ArgumentParser(description="Attendance server: the reference's routes and flags on the HIP path")
    p.add_argument("--gallery", type=str, default="gallery/adaface_ir101.pkl", help="gallery file of the enrolled students")
    p.add_argument("--threshold", type=float, default=0.4, help="top-1 cosine at or above which a track is recognised")
    p.add_argument("--output_dir", type=str, default="sessions", help="folder under which the session folders are made")
    p.add_argument("--session_name", type=str, default=None, help="open this session at start-up (default: the client names it)")
    p.add_argument("--recognition_interval", type=int, default=30, help="stored in session.json; the tracker does not read it")
    p.add_argument("--max_attempts", type=int, default=3, help="attempts per track and cooldown cycle")
    p.add_argument("--enable_perf_monitor", action="store_true", default=True, help="Accepted; no monitor is built")
    p.add_argument("--enable_gpu_monitor", action="store_true", default=True, help="Accepted; no monitor is built")
    p.add_argument("--use_gpu", action="store_true", default=True, help="Use the GPU (there is no CPU path)")
    p.add_argument("--use_cpu", action="store_true", help="Refused: there is no CPU path")
    p.add_argument("--model_type", type=str, default="adaface", choices=["adaface", "arcface"])
    p.add_argument("--architecture", type=str, default="ir_101", choices=["ir_50", "ir_101"])
    p.add_argument("--host", type=str, default="0.0.0.0", help="address to listen on")
    p.add_argument("--port", type=int, default=5000, help="port to listen on")
    p.add_argument("--require_session_name", action="store_true", help="stored; as in the reference nothing reads it")
    p.add_argument("--frame_skip", type=int, default=3, help="Accepted for the client's sake; not read")
    args = p.parse_args(argv)
    if args.use_cpu:
        raise SystemExit("this server runs on a HIP device only (no CPU fallback)")
    server = FaceRecognitionServer(gallery_path=args.gallery, similarity_threshold=args.threshold,
                                   output_dir=args.output_dir, session_name=args.session_name,
                                   recognition_interval=args.recognition_interval,
                                   max_recognition_attempts=args.max_attempts,
                                   enable_performance_monitoring=args.enable_perf_monitor,
                                   enable_gpu_monitoring=args.enable_gpu_monitor, model_type=args.model_type,
                                   architecture=args.architecture, require_session_name=args.require_session_name)
    print(f"\nStarting server on {args.host}:{args.port}...")
    create_app(server).run(host=args.host, port=args.port, threaded=True)


if __name__ == "__main__":
    main()
