"""What the live loop (face_recognition_live.py) and the attendance server (face_recognition_server.py)
have in common.  The reference copied one module from the other; here the copy exists once:

* ``selection_key`` and ``PROCESSOR_CONFIG``;
* ``TrackRecords``: the per-track dicts and the ring of both ``LiveRecognitionTracker`` classes.  When
  a track is due (``should_recognize``) is each tracker's own;
* ``AttendanceSession``: ``session.json`` / ``attendance.json``, the attendance merge, the result dict
  and the session close of ``LiveFaceRecognition`` and ``FaceRecognitionServer``.  How a face is saved
  and what becomes of an attempt's result (``_save_face_image``, ``_settle``) is each class's own;
* ``_resolve``: the attempts the reference makes out of a kernel's speculative candidates, behind
  ``resolve_attempts`` and ``resolve_server_attempts``.

Line numbers in the docstrings are face_recognition_live.py's, then face_recognition_server.py's.
"""
from __future__ import annotations

import json
import os
from collections import deque
from datetime import datetime
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np

# the FaceProcessor settings of both sessions (:114-128, :170-184)
PROCESSOR_CONFIG = dict(output_size=112, det_size=(640, 640), det_thresh=0.5,
                        quality_filter_config={"min_det_score": 0.5, "min_face_size": 40, "max_yaw": 60,
                                               "max_pitch": 45, "max_roll": 45, "check_blur": True,
                                               "blur_threshold": 50})


def selection_key(det_score: float, blur_score: float) -> float:
    """``LiveRecognitionTracker.get_best_frame``'s ``quality_score`` on plain doubles."""
    blur_normalized = min(blur_score / 100.0, 1.0)
    return det_score * blur_normalized


def _resolve(ordinals: Iterable[int], track_key: Sequence, attempt, best,
             recognise: Callable[[List[int]], List[List]], similarity_threshold: float, max_attempts: int,
             trace: Optional[set] = None):
    """For every ordinal k of ``ordinals``, in the order given: the ``best`` detections of the
    candidates with ``attempt == k`` whose track is not yet recognised go through one
    ``recognise(list of detection indices)`` call, which returns per entry the ``gallery.search`` list
    ``[(student_id, name, score), ...]``.  A success drops the track's later candidates; a failure on
    the last attempt of a cycle (``k % max_attempts == max_attempts - 1``) is an ``unrecognized``
    event.  An empty ``matches`` (empty gallery) counts as an attempt and yields nothing, as in the
    reference.  Returns ``(log, events)`` in detection order: ``log`` = the attempts made, ``{'det',
    'track', 'attempt', 'best', 'matches'}``; ``events`` = the same with ``'type'`` ('recognized' |
    'unrecognized')."""
    attempt = np.asarray(attempt).reshape(-1)
    best = np.asarray(best).reshape(-1)
    max_attempts = int(max_attempts)
    ev = trace.add if trace is not None else (lambda name: None)
    recognized: Dict = {}
    log, events = [], []
    for k in ordinals:
        cand = [int(d) for d in np.flatnonzero(attempt == k) if track_key[d] not in recognized]
        if not cand:
            continue
        found = recognise([int(best[d]) for d in cand])
        for d, matches in zip(cand, found):
            entry = {"det": d, "track": track_key[d], "attempt": k, "best": int(best[d]), "matches": list(matches)}
            log.append(entry)
            if not matches:
                continue
            if matches[0][2] >= similarity_threshold:
                recognized[track_key[d]] = k
                events.append(dict(entry, type="recognized"))
            elif k % max_attempts == max_attempts - 1:
                ev("attempts_exhausted")
                if k >= max_attempts:
                    ev("second_cycle_unrecognized")
                events.append(dict(entry, type="unrecognized"))
    if trace is not None:
        for d in np.flatnonzero(attempt >= 0):
            k = recognized.get(track_key[d])
            if k is not None and k >= 1 and attempt[d] > k:
                ev("recognized_later_then_silent")
    log.sort(key=lambda e: e["det"])
    events.sort(key=lambda e: e["det"])
    return log, events


class TrackRecords:
    """What both trackers know of every track id (:18-80, :23-124): its outcome, its attempts, a ring of
    its last ``buffer_size`` faces, first and last timestamp."""

    def __init__(self, recognition_interval, max_attempts, buffer_size):
        self.recognition_interval = recognition_interval
        self.max_attempts = max_attempts
        self.buffer_size = buffer_size
        self.recognized_tracks: Dict = {}      # track id -> the result dict that resolved it
        self.recognition_attempts: Dict = {}   # track id -> attempts (the server: of the current cycle)
        self.track_frame_buffers: Dict = {}    # track id -> deque of face dicts, oldest first
        self.track_first_seen: Dict = {}       # ISO timestamps
        self.track_last_seen: Dict = {}

    def add_frame(self, track_id, face_data: Dict, timestamp: str):
        ring = self.track_frame_buffers.get(track_id)
        if ring is None:
            ring = self.track_frame_buffers[track_id] = deque(maxlen=self.buffer_size)
            self.track_first_seen[track_id] = timestamp
        ring.append(face_data)
        self.track_last_seen[track_id] = timestamp

    def get_best_frame(self, track_id) -> Optional[Dict]:
        """The buffered face with the largest ``selection_key``; the oldest of equal keys."""
        ring = self.track_frame_buffers.get(track_id)
        if not ring:
            return None
        return max(ring, key=lambda face: selection_key(face.get("det_score", 0),
                                                        face.get("quality_metrics", {}).get("blur_score", 0)))

    def mark_recognized(self, track_id, student_info: Dict):
        self.recognized_tracks[track_id] = student_info

    def increment_attempts(self, track_id):
        self.recognition_attempts[track_id] = 1 + self.recognition_attempts.get(track_id, 0)

    def get_track_duration(self, track_id) -> float:
        try:
            first, last = self.track_first_seen[track_id], self.track_last_seen[track_id]
        except KeyError:
            return 0.0
        return (datetime.fromisoformat(last) - datetime.fromisoformat(first)).total_seconds()


class AttendanceSession:
    """The session folder of ``LiveFaceRecognition`` and ``FaceRecognitionServer``.  A subclass sets
    ``verbose``, ``trace``, ``similarity_threshold``, ``recognition_interval``,
    ``max_recognition_attempts``, ``session_name`` and ``session_dir``, and opens the session with
    ``_open_session(tracker)``."""

    PROCESSOR_CONFIG = PROCESSOR_CONFIG
    SUMMARY_INDENT = ""  # before the per-student and per-track lines of the closing summary

    def _print(self, *args, **kw) -> None:
        if self.verbose:
            print(*args, **kw)

    def _note(self, name: str) -> None:
        """``trace`` (a set, or None): the tests' record of the situations the session met."""
        if self.trace is not None:
            self.trace.add(name)

    # -- the models: each constructor calls these in the reference's order ---------------------------
    def _load_processor(self, processor, device) -> None:
        if processor is None:
            from .face_recognition import FaceProcessor
            processor = FaceProcessor(device=device, **self.PROCESSOR_CONFIG)
        self.face_processor = processor

    def _load_embedder(self, embedder, architecture, model_path, model_type, device) -> None:
        if embedder is None:
            from .face_embedder import FaceEmbedder
            embedder = FaceEmbedder(architecture=architecture, model_path=model_path, model_type=model_type,
                                    device=device)
        self.embedder = embedder
        self.model_type = model_type
        self.architecture = architecture

    def _load_gallery(self, gallery, gallery_path) -> None:
        if gallery is None:
            from .gallery_manager import GalleryManager
            gallery = GalleryManager(gallery_path=gallery_path, device=self.embedder.device, verbose=self.verbose)
        self.gallery = gallery
        if hasattr(self.gallery, "attach_handle") and hasattr(self.embedder, "model"):
            self.gallery.attach_handle(self.embedder.model)
        num_students = len(self.gallery.get_all_students())
        self._print(f"Loaded {num_students} enrolled students")
        if num_students == 0:
            self._print("\nWARNING: Gallery is empty! Please enroll students first.")

    # -- the session and its files (:173-247, :230-312) -----------------------------------------------
    def _open_session(self, tracker: TrackRecords) -> None:
        """``session_dir`` with its two face folders, a fresh tracker, the counters at zero, the files."""
        os.makedirs(self.session_dir, exist_ok=True)
        self.tracker = tracker
        self.recognized_faces_dir = os.path.join(self.session_dir, "recognized_faces")
        self.unrecognized_faces_dir = os.path.join(self.session_dir, "unrecognized_faces")
        os.makedirs(self.recognized_faces_dir, exist_ok=True)
        os.makedirs(self.unrecognized_faces_dir, exist_ok=True)
        self.session_start = datetime.now()
        self.frame_count = 0
        self.total_faces_detected = 0
        self.total_recognition_attempts = 0
        self._init_session_files()

    def _init_session_files(self):
        session_data = {
            "session_id": self.session_name,
            "start_time": self.session_start.isoformat(),
            "end_time": None,
            "status": "active",
            "settings": {
                "similarity_threshold": self.similarity_threshold,
                "recognition_interval": self.recognition_interval,
                "max_recognition_attempts": self.max_recognition_attempts,
            },
            "statistics": {
                "total_frames_processed": 0,
                "total_faces_detected": 0,
                "total_recognition_attempts": 0,
                "unique_students_recognized": 0,
                "unrecognized_tracks": 0,
            },
        }
        attendance_data = {
            "session_id": self.session_name,
            "last_updated": datetime.now().isoformat(),
            "recognized": [],
            "unrecognized": [],
        }
        self._write_session(session_data)
        self._write_attendance(attendance_data)

    def _write_session(self, data: Dict):
        with open(os.path.join(self.session_dir, "session.json"), "w") as f:
            json.dump(data, f, indent=2)

    def _write_attendance(self, data: Dict):
        with open(os.path.join(self.session_dir, "attendance.json"), "w") as f:
            json.dump(data, f, indent=2)

    def _read(self, name: str) -> Dict:
        with open(os.path.join(self.session_dir, name), "r") as f:
            return json.load(f)

    def _result_of(self, matches, track_id, face_data: Dict, timestamp: str) -> Optional[Dict]:
        """The result dict of ``_recognize_face`` (:296-318, :314-347) from ``gallery.search``'s list for
        the face ``face_data`` (its ``det_score`` and ``quality_metrics``)."""
        if len(matches) == 0:
            return None
        student_id, name, score = matches[0]
        return {
            "student_id": student_id,
            "name": name,
            "confidence": float(score),
            "track_id": track_id,
            "recognized": bool(score >= self.similarity_threshold),
            "top_matches": [{"student_id": sid, "name": n, "score": float(s)} for sid, n, s in matches],
            "timestamp": timestamp,
            "detection_quality": {"det_score": float(face_data["det_score"]),
                                  "blur_score": face_data["quality_metrics"].get("blur_score", 0)},
        }

    def _update_attendance(self, events: List[tuple]):
        """:458-506, :478-526: merge a frame's or a request's ``(type, result)`` events into
        ``attendance.json``.  A student is listed once; a later track that recognises the same student
        only raises the entry's confidence (and the detection quality that goes with it).  On the server
        a track may be listed as unrecognized once per cooldown cycle."""
        attendance = self._read("attendance.json")
        recognized, unrecognized = attendance["recognized"], attendance["unrecognized"]
        for kind, result in events:
            tid = result["track_id"]
            label = f"track_{tid:04d}"
            first_seen = self.tracker.track_first_seen.get(tid, result["timestamp"])
            duration = self.tracker.get_track_duration(tid)
            saved = result.get("saved_face_path", "")
            if kind == "recognized":
                known = [s for s in recognized if s["student_id"] == result["student_id"]]
                if not known:
                    recognized.append({"student_id": result["student_id"], "name": result["name"],
                                       "first_seen": first_seen, "confidence": result["confidence"], "track_id": label,
                                       "duration_seconds": duration, "detection_quality": result["detection_quality"],
                                       "saved_face_path": saved})
                elif result["confidence"] > known[0]["confidence"]:
                    known[0].update(confidence=result["confidence"], detection_quality=result["detection_quality"])
                    self._note("second_track_higher")
                else:
                    self._note("second_track_lower")
            elif kind == "unrecognized":
                best_match = {key: result[key] for key in ("name", "student_id", "confidence")}
                unrecognized.append({"track_id": label, "first_seen": first_seen, "duration_seconds": duration,
                                     "best_match": best_match, "reason": "below_threshold",
                                     "threshold": self.similarity_threshold,
                                     "attempts": self.tracker.recognition_attempts.get(tid, 0),
                                     "top_matches": result["top_matches"], "saved_face_path": saved})
        attendance["last_updated"] = datetime.now().isoformat()
        self._write_attendance(attendance)

    # -- the session close (:632-684, :538-584) ---------------------------------------------------------
    def _rate_statistics(self, seconds: float) -> Dict:
        """The statistics a class adds after the five common ones; their summary lines are
        ``_rate_summary``'s."""
        return {}

    def _rate_summary(self, statistics: Dict) -> str:
        return ""

    def _close_session(self) -> Dict:
        """Close ``session.json`` (end time, status, duration, the statistics), print the summary and
        return the dict."""
        ended = datetime.now()
        seconds = (ended - self.session_start).total_seconds()
        session, attendance = self._read("session.json"), self._read("attendance.json")
        session.update(end_time=ended.isoformat(), status="completed", duration_seconds=seconds)
        session["statistics"] = {
            "total_frames_processed": self.frame_count,
            "total_faces_detected": self.total_faces_detected,
            "total_recognition_attempts": self.total_recognition_attempts,
            "unique_students_recognized": len(attendance["recognized"]),
            "unrecognized_tracks": len(attendance["unrecognized"]),
            **self._rate_statistics(seconds),
        }
        self._write_session(session)
        rule, indent = "=" * 70, self.SUMMARY_INDENT
        self._print(f"\n{rule}\nFINALIZING SESSION\n{rule}")
        self._print(f"\nSession: {self.session_name}\nDuration: {seconds:.1f} seconds\n"
                    f"Frames processed: {self.frame_count}{self._rate_summary(session['statistics'])}")
        self._print(f"\nRecognized students: {len(attendance['recognized'])}")
        for s in attendance["recognized"]:
            self._print(f"{indent}{s['name']} ({s['student_id']}) - confidence: {s['confidence']:.3f}")
        self._print(f"\nUnrecognized tracks: {len(attendance['unrecognized'])}")
        for t in attendance["unrecognized"]:
            best = t["best_match"]
            self._print(f"{indent}{t['track_id']} - best match: {best['name']} ({best['confidence']:.3f})")
        self._print(f"\nOutput directory: {self.session_dir}\n{rule}\n")
        return session
