"""``SimpleTracker`` / ``FrameAccumulator`` / ``CameraFaceCapture`` — the reference's capture
session (face_detection.py:11-405): frames in, ``track_XXX/frame_NNN.jpg`` + ``metadata.json``
folders out, which is what ``FaceMatcher.process_capture_directory`` reads.

``SimpleTracker`` and ``FrameAccumulator`` are the per-frame host classes with the reference's
names, arguments, dict keys and defaults (no scipy: the centroid distances are plain numpy).
``capture_tracks_host`` states the same session in integers for a whole clip; it is the contract of
the ``fr_capture_tracks`` kernel, which runs the tracker and the accumulator of many clips
(cameras) in one launch.  ``CameraFaceCapture.process_clip`` is the reference's ``process_frame``
loop for a whole clip: the frames at ``frame_count % skip_frames == 0`` are detected as one batch,
aligned, blur-scored and gated with the ``FaceProcessor`` pieces, boxes / metrics / validity go up
once, one ``capture_tracks`` call decides every track, and the saved crops are gathered per track
on the device.  ``recognize_clip`` hands those tracks to ``FaceMatcher.match_tracks``.

Notes on parity:

* Images are written with PIL (JPEG quality 95, ``cv2.imwrite``'s default).  The JPEG bytes
  against ``cv2.imwrite`` are UNPINNED (cv2 is not a dependency); the decoded crops differ from
  the written ones by JPEG loss only, as in the reference.
* The tracker compares ``sqrt`` distances in the reference and integers ``q = 4 d^2`` here.  The
  order is the same: two different ``q`` in range differ in ``sqrt`` by more than 1e-5 while an ulp
  is about 1e-12, and the threshold is ``q_limit(max_distance)``, for which ``q < q_limit`` is
  ``sqrt(q / 4.0) < max_distance`` bit for bit.
* The quality score takes the metrics as float64 (``process_clip`` converts them).  That is the
  reference under NumPy 1.x scalar promotion; under NumPy 2 the ``np.float32`` pose angles of
  float32 landmarks keep the reference's pose term in float32, a difference of about 1e-8 in the
  score.  Metrics must be finite (``ValueError``).
* ``run()`` and ``draw_visualizations`` (camera and window I/O through cv2) are not provided; a
  call of ``process_clip`` is one session (no tracker state is carried between calls).
"""
from __future__ import annotations

import json
import math
import os
from collections import defaultdict
from datetime import datetime
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# include/frhip.h FR_CAPTURE_*
CAPTURE_MAX_FACES = 128
CAPTURE_MAX_TRACKS = 128
CAPTURE_MAX_DETS = 4096
CAPTURE_MAX_TARGET = 64
CAPTURE_COORD_MAX = 1 << 20
CAPTURE_ERR_TRACKS, CAPTURE_ERR_COORD = 1, 2

METRIC_KEYS = ("blur_score", "yaw", "pitch", "roll")  # metrics columns 1..4; column 0 is det_score


def q_limit(max_distance: float) -> int:
    """The smallest integer ``q >= 0`` with ``sqrt(q / 4.0) >= max_distance`` in double, where
    ``q = (sx_t - sx_d)^2 + (sy_t - sy_d)^2`` is 4 x a squared centroid distance: ``q < q_limit`` is
    the reference's ``distance < max_distance``.  0 for ``max_distance <= 0`` or NaN (nothing
    matches); past every ``q`` in range for a ``max_distance`` beyond every distance in range."""
    md = float(max_distance)
    if not md > 0.0:
        return 0
    if md >= 4194304.0:
        return 1 << 46
    q = int(math.floor(4.0 * md * md))
    while q > 0 and math.sqrt((q - 1) / 4.0) >= md:
        q -= 1
    while math.sqrt(q / 4.0) < md:
        q += 1
    return q


class SimpleTracker:
    """face_detection.py:11-121: greedy nearest-centroid tracker, one ``update`` per frame."""

    def __init__(self, max_disappeared=30, max_distance=50):
        self.next_track_id = 1
        self.tracks: Dict[int, Dict] = {}
        self.max_disappeared = max_disappeared
        self.max_distance = max_distance

    def compute_centroid(self, bbox):
        x1, y1, x2, y2 = bbox
        return np.array([(x1 + x2) / 2, (y1 + y2) / 2])

    def compute_iou(self, bbox1, bbox2):
        x1_1, y1_1, x2_1, y2_1 = bbox1
        x1_2, y1_2, x2_2, y2_2 = bbox2
        x_left, y_top = max(x1_1, x1_2), max(y1_1, y1_2)
        x_right, y_bottom = min(x2_1, x2_2), min(y2_1, y2_2)
        if x_right < x_left or y_bottom < y_top:
            return 0.0
        intersection = (x_right - x_left) * (y_bottom - y_top)
        area1 = (x2_1 - x1_1) * (y2_1 - y1_1)
        area2 = (x2_2 - x1_2) * (y2_2 - y1_2)
        union = area1 + area2 - intersection
        return intersection / union if union > 0 else 0

    def _open(self, detection) -> int:
        track_id = self.next_track_id
        self.next_track_id += 1
        self.tracks[track_id] = {"bbox": detection["bbox"], "centroid": self.compute_centroid(detection["bbox"]),
                                 "disappeared": 0, "last_seen": datetime.now()}
        return track_id

    def _age(self, track_ids) -> None:
        for track_id in track_ids:
            self.tracks[track_id]["disappeared"] += 1
            if self.tracks[track_id]["disappeared"] > self.max_disappeared:
                del self.tracks[track_id]

    def update(self, detections: Sequence[Dict]) -> List[Tuple[int, Dict]]:
        """The reference's ``(track_id, detection)`` list: the matched pairs in the order the
        greedy loop takes them, then the new tracks in detection order."""
        if len(detections) == 0:
            self._age(list(self.tracks.keys()))
            return []
        if len(self.tracks) == 0:
            return [(self._open(d), d) for d in detections]
        track_ids = list(self.tracks.keys())
        track_centroids = np.array([self.tracks[tid]["centroid"] for tid in track_ids], dtype=np.float64)
        detection_centroids = np.array([self.compute_centroid(d["bbox"]) for d in detections], dtype=np.float64)
        # scipy's cdist (euclidean): sqrt(dx^2 + dy^2); half-integer centroids make the sum exact
        diff = track_centroids[:, None, :] - detection_centroids[None, :, :]
        distances = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1])
        matched_tracks, matched_detections = set(), set()
        results = []
        while distances.size > 0 and distances.min() < self.max_distance:
            min_idx = int(distances.argmin())
            track_idx, det_idx = divmod(min_idx, len(detections))
            if track_idx in matched_tracks or det_idx in matched_detections:
                distances[track_idx, det_idx] = np.inf
                continue
            track_id, detection = track_ids[track_idx], detections[det_idx]
            self.tracks[track_id].update({"bbox": detection["bbox"],
                                          "centroid": self.compute_centroid(detection["bbox"]),
                                          "disappeared": 0, "last_seen": datetime.now()})
            results.append((track_id, detection))
            matched_tracks.add(track_idx)
            matched_detections.add(det_idx)
            distances[track_idx, det_idx] = np.inf
        self._age([tid for idx, tid in enumerate(track_ids) if idx not in matched_tracks])
        for idx, detection in enumerate(detections):
            if idx not in matched_detections:
                results.append((self._open(detection), detection))
        return results


class FrameAccumulator:
    """face_detection.py:123-228: the first ``target_frames`` good frames of every track, saved
    best first as ``track_%03d/frame_%03d.jpg`` + ``metadata.json``.  Images are written with PIL;
    the JPEG bytes against ``cv2.imwrite`` are unpinned."""

    def __init__(self, target_frames=12, min_quality_score=0.5, output_dir="output/camera_captures",
                 verbose: bool = True):
        self.target_frames = target_frames
        self.min_quality_score = min_quality_score
        self.output_dir = output_dir
        self.verbose = verbose
        os.makedirs(output_dir, exist_ok=True)
        self.accumulated_frames = defaultdict(list)
        self.completed_tracks = set()
        self.metadata: Dict[int, Dict] = {}

    def compute_quality_score(self, face_dict):
        metrics = face_dict["quality_metrics"]
        det_score = face_dict["det_score"]
        blur_score = metrics.get("blur_score", 0)
        normalized_blur = min(blur_score / 200.0, 1.0)
        yaw = abs(metrics.get("yaw", 0))
        pitch = abs(metrics.get("pitch", 0))
        roll = abs(metrics.get("roll", 0))
        pose_score = 1.0 - (yaw / 90.0 + pitch / 90.0 + roll / 90.0) / 3.0
        pose_score = max(0, pose_score)
        return det_score * 0.4 + normalized_blur * 0.3 + pose_score * 0.3

    def add_frame(self, track_id, face_dict, frame_rgb=None):
        if track_id in self.completed_tracks:
            return True
        quality = self.compute_quality_score(face_dict)
        if quality < self.min_quality_score:
            return False
        self.accumulated_frames[track_id].append({
            "aligned_face": face_dict["aligned_face"], "quality_score": quality, "det_score": face_dict["det_score"],
            "metrics": face_dict["quality_metrics"], "timestamp": datetime.now().isoformat()})
        if len(self.accumulated_frames[track_id]) >= self.target_frames:
            if track_id not in self.completed_tracks:
                self.save_track(track_id)
            return True
        return False

    def save_track(self, track_id, write: bool = True):
        """:181-222.  ``write=False`` builds the metadata and marks the track without touching the
        disk (``CameraFaceCapture.process_clip(save=False)``)."""
        if track_id in self.completed_tracks:
            return
        frames = self.accumulated_frames[track_id]
        if len(frames) == 0:
            return
        frames.sort(key=lambda x: x["quality_score"], reverse=True)
        frames_to_save = frames[:self.target_frames]
        track_dir = os.path.join(self.output_dir, f"track_{track_id:03d}")
        saved_files = [f"frame_{idx:03d}.jpg" for idx in range(len(frames_to_save))]
        if write:
            from PIL import Image
            os.makedirs(track_dir, exist_ok=True)
            for filename, frame_data in zip(saved_files, frames_to_save):
                # the reference converts RGB to BGR for cv2.imwrite: the file holds the RGB picture
                Image.fromarray(np.ascontiguousarray(frame_data["aligned_face"], dtype=np.uint8)).save(
                    os.path.join(track_dir, filename), quality=95)
        metadata = {
            "track_id": track_id,
            "num_frames": len(frames_to_save),
            "avg_quality": float(np.mean([f["quality_score"] for f in frames_to_save])),
            "avg_det_score": float(np.mean([f["det_score"] for f in frames_to_save])),
            "saved_at": datetime.now().isoformat(),
            "files": saved_files,
        }
        if write:
            with open(os.path.join(track_dir, "metadata.json"), "w") as f:
                json.dump(metadata, f, indent=2)
        self.metadata[track_id] = metadata
        self.completed_tracks.add(track_id)
        if self.verbose:
            print(f"\nSaved {len(frames_to_save)} frames for track_{track_id:03d}")
            print(f"  Avg quality: {metadata['avg_quality']:.3f}")
            print(f"  Location: {track_dir}")

    def get_status(self, track_id):
        if track_id in self.completed_tracks:
            return "completed"
        count = len(self.accumulated_frames[track_id])
        return f"{count}/{self.target_frames}"


def quality_score(det_score: float, blur_score: float, yaw: float, pitch: float, roll: float) -> float:
    """``FrameAccumulator.compute_quality_score`` on plain doubles, in its order of operations."""
    normalized_blur = min(blur_score / 200.0, 1.0)
    pose_score = 1.0 - (abs(yaw) / 90.0 + abs(pitch) / 90.0 + abs(roll) / 90.0) / 3.0
    pose_score = max(0, pose_score)
    return det_score * 0.4 + normalized_blur * 0.3 + pose_score * 0.3


def capture_tracks_host(bbox, metrics, valid, frame_offsets, max_disappeared: int = 30, max_distance: float = 50,
                        target_frames: int = 12, min_quality_score: float = 0.5, save_partial: bool = False,
                        trace: Optional[set] = None):
    """What ``fr_capture_tracks`` computes for one clip, in plain Python: ``bbox`` int [n,4],
    ``metrics`` float64 [n,5] (det_score, blur_score, yaw, pitch, roll), ``valid`` [n]; frame f =
    detections ``[frame_offsets[f], frame_offsets[f+1])``.  Returns ``(track_id int32 [n], quality
    float64 [n], slot int32 [n], [tracks opened, tracks completed, frames saved, error])``.

    ``trace`` (a set) collects the names of the situations the clip went through (ties, the
    distance and disappearance edges, list-order cases, quality edges, ...): the tests use it to
    show that a fixture reaches them."""
    bbox = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    metrics = np.asarray(metrics, dtype=np.float64).reshape(-1, 5)
    fo = [int(v) for v in np.asarray(frame_offsets).reshape(-1)]
    n = bbox.shape[0]
    valid = np.asarray(valid).reshape(-1)
    ev = trace.add if trace is not None else (lambda name: None)
    quality = np.array([quality_score(*(float(v) for v in m)) for m in metrics], dtype=np.float64).reshape(n)
    track_id = np.zeros(n, np.int32)
    slot = np.full(n, -1, np.int32)
    if n and int(np.abs(bbox).max()) > CAPTURE_COORD_MAX:
        return track_id, quality, slot, [0, 0, 0, CAPTURE_ERR_COORD]
    limit = q_limit(max_distance)
    at_limit = limit > 0 and math.sqrt(limit / 4.0) == float(max_distance)
    # ---- the tracker: the live list in dict order, [id, sx, sy, disappeared]
    live: List[List[int]] = []
    next_id = 1
    deleted_before_survivor = False  # a deletion has moved a later track up the list
    for f in range(len(fo) - 1):
        dets = [(int(b[0] + b[2]), int(b[1] + b[3])) for b in bbox[fo[f]:fo[f + 1]]]
        nd, nt = len(dets), len(live)
        if nd == 0:
            ev("empty_first" if f == 0 else "empty_middle" if nt else "empty_no_tracks")
        elif nt == 0 and next_id > 1:
            ev("frame_after_all_died")
        if nd and nt:
            ev("more_dets" if nd > nt else "more_tracks" if nt > nd else "same_count")
        t_matched, d_matched = [False] * nt, [False] * nd
        while True:
            best = None
            for tp in range(nt):
                if t_matched[tp]:
                    continue
                for di in range(nd):
                    if d_matched[di]:
                        continue
                    q = (live[tp][1] - dets[di][0]) ** 2 + (live[tp][2] - dets[di][1]) ** 2
                    if q == limit and at_limit:
                        ev("at_max_distance")
                    if q < limit and (best is None or q < best[0]):  # the first of equal q: smallest flat index
                        best = (q, tp, di)
            if best is None:
                break
            q, tp, di = best
            if trace is not None:
                for tp2 in range(nt):
                    for di2 in range(nd):
                        if t_matched[tp2] or d_matched[di2] or (tp2, di2) == (tp, di):
                            continue
                        if (live[tp2][1] - dets[di2][0]) ** 2 + (live[tp2][2] - dets[di2][1]) ** 2 == q:
                            if tp2 == tp:
                                ev("tie_two_dets_one_track")
                            if di2 == di:
                                ev("tie_two_tracks_one_det")
                if q >= limit - 3:  # q = 3 (mod 4) is no sum of two squares, so limit - 1 may be out of reach
                    ev("just_under_max_distance")
                if live[tp][3] == max_disappeared and max_disappeared > 0:
                    ev("kept_at_max_disappeared")
            t_matched[tp] = d_matched[di] = True
            live[tp][1], live[tp][2], live[tp][3] = dets[di][0], dets[di][1], 0
            track_id[fo[f] + di] = live[tp][0]
        kept = []
        for tp, tr in enumerate(live):
            if not t_matched[tp]:
                tr[3] += 1
                if tr[3] > max_disappeared:
                    ev("deleted")
                    deleted_before_survivor = deleted_before_survivor or any(
                        t_matched[j] or live[j][3] + 1 <= max_disappeared for j in range(tp + 1, nt))
                    continue
            kept.append(tr)
        opened = [di for di in range(nd) if not d_matched[di]]
        if opened and deleted_before_survivor:
            ev("delete_then_append")
        if opened and trace is not None and "deleted" in trace:
            ev("new_id_after_deletion")
        if len(kept) + len(opened) > CAPTURE_MAX_TRACKS:
            return np.zeros(n, np.int32), quality, slot, [0, 0, 0, CAPTURE_ERR_TRACKS]
        for rank, di in enumerate(opened):
            kept.append([next_id + rank, dets[di][0], dets[di][1], 0])
            track_id[fo[f] + di] = next_id + rank
        next_id += len(opened)
        live = kept
    # ---- the accumulator
    passes = [bool(valid[i]) and not (quality[i] < min_quality_score) for i in range(n)]
    accepted: Dict[int, List[int]] = defaultdict(list)
    for i in range(n):
        m = metrics[i]
        if trace is not None:
            if not valid[i]:
                ev("invalid_face")
            if m[1] > 200.0:
                ev("blur_over_200")
            if 1.0 - (abs(m[2]) / 90.0 + abs(m[3]) / 90.0 + abs(m[4]) / 90.0) / 3.0 < 0:
                ev("pose_clamped")
            if min(m[2], m[3], m[4]) < 0:
                ev("negative_angle")
            if valid[i] and quality[i] == min_quality_score:
                ev("quality_equals_minimum")
        if not passes[i]:
            continue
        got = accepted[int(track_id[i])]
        if len(got) < target_frames:
            got.append(i)
        elif quality[i] > max(quality[j] for j in got):
            ev("better_frame_after_completion")
    completed = saved = 0
    for tid, got in accepted.items():
        full = len(got) == target_frames
        completed += full
        if len({float(quality[i]) for i in got}) < len(got):
            ev("equal_qualities_in_track")
        if not full:
            ev("partial_saved" if save_partial else "partial_dropped")
        if not (full or save_partial):
            continue
        order = sorted(got, key=lambda i: quality[i], reverse=True)  # stable: equal qualities in frame order
        for rank, i in enumerate(order):
            slot[i] = rank
        saved += len(order)
    return track_id, quality, slot, [next_id - 1, completed, saved, 0]


class CameraFaceCapture:
    """face_detection.py:230-405 without the camera: ``process_clip`` is the ``process_frame`` loop
    of one session over a clip that is already in memory, with the tracker and the accumulator on
    the GPU.  ``processor`` (a ``FaceProcessor``, or anything with its ``detector`` / ``aligner`` /
    ``quality_filter``) defaults to the reference's settings (:243-256)."""

    PROCESSOR_CONFIG = dict(output_size=224, det_size=(640, 640), det_thresh=0.4,
                            quality_filter_config={"min_det_score": 0.6, "min_face_size": 60, "max_yaw": 45,
                                                   "max_pitch": 30, "max_roll": 30, "check_blur": True,
                                                   "blur_threshold": 100})

    def __init__(self, output_dir="output/camera_captures", skip_frames=5, target_frames_per_person=12,
                 min_quality_score=0.5, processor=None, device=None, verbose: bool = True,
                 device_chain: bool = False):
        import torch
        from .face_recognition import FaceProcessor
        self.skip_frames = skip_frames
        # True: a clip's sampled frames go through detect, align, blur and the quality gate on the
        # device in one pass (face_recognition.device_chain) instead of per-frame calls and a host gate
        self.device_chain = bool(device_chain)
        self.frame_count = 0
        self.verbose = verbose
        self.processor = processor if processor is not None else FaceProcessor(device=device,
                                                                               **self.PROCESSOR_CONFIG)
        self.device = self.processor.aligner._ops.device if device is None else torch.device(device)
        self.tracker = SimpleTracker(max_disappeared=30, max_distance=80)
        self.accumulator = FrameAccumulator(target_frames=target_frames_per_person,
                                            min_quality_score=min_quality_score, output_dir=output_dir,
                                            verbose=verbose)
        self.accumulators = [self.accumulator]  # one per clip of the last process_clip call
        self.total_tracks = [0]

    # -- detect -> align -> blur -> gate for the sampled frames of one clip ------------------
    def _faces_of_clip(self, frames):
        """Per sampled frame the reference's ``process_numpy(frame, return_all=True)`` list (its
        order: descending det_score x blur_score), with the aligned crops left on the device:
        ``(frame numbers, [[face dict, ...], ...], crops uint8 [total,S,S,3] on the device)`` where
        a face dict carries ``'crop_row'`` instead of ``'aligned_face'``.

        With ``device_chain`` the sampled frames run detect_device -> align_device ->
        blur_scores_device -> gate_device in one pass with one copy to the host, the order comes from
        the gate's ranks, ``crops`` holds one crop per slot ([frames * max_faces,S,S,3]) and
        ``'crop_row'`` is the slot index.  The same faces, order and flags; yaw and roll as
        ``quality_gate_host`` states them (within 1e-4 degrees of the host gate's).  A detection whose
        similarity fit fails, where the host chain raises, is ``is_valid: False`` there."""
        import torch
        p = self.processor
        if isinstance(frames, torch.Tensor):
            clip = frames
        else:
            clip = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8))
        if clip.dtype != torch.uint8 or clip.dim() != 4 or clip.shape[3] != 3:
            raise ValueError("expected a uint8 [n,H,W,3] RGB clip")
        picked = [i for i in range(clip.shape[0]) if i % self.skip_frames == 0]
        S = p.aligner.output_size
        if not picked:
            return picked, [], torch.empty((0, S, S, 3), dtype=torch.uint8, device=self.device)
        dev = clip[picked].to(self.device).contiguous()
        if getattr(self, "device_chain", False):
            from .face_recognition import chain_faces, device_chain
            host, _gate, crops = device_chain(p.detector, p.aligner, p.quality_filter, dev)
            out = []
            for f in range(len(picked)):
                faces = chain_faces(p.quality_filter, host, f)
                for x in faces:
                    x["crop_row"] = x.pop("slot")
                out.append(faces)
            return picked, out, crops
        if hasattr(p.detector, "detect_batch"):
            per_frame = p.detector.detect_batch(dev)
        else:  # the reference's detector contract: one host image at a time
            host = dev.cpu().numpy()
            per_frame = [p.detector.detect(host[i]) for i in range(len(picked))]
        crops = [p.aligner.align_batch(dev[i], np.stack([f["landmarks"] for f in faces]))
                 for i, faces in enumerate(per_frame) if len(faces)]
        crops = torch.cat(crops) if crops else torch.empty((0, S, S, 3), dtype=torch.uint8, device=self.device)
        blur = p.quality_filter.compute_blur_scores(crops) if p.quality_filter.check_blur and len(crops) else None
        out, row = [], 0
        for faces in per_frame:
            results = []
            for face in faces:
                ok, q = p.quality_filter.is_valid(face, None, None if blur is None else float(blur[row]))
                results.append({"crop_row": row, "bbox": face["bbox"], "landmarks": face["landmarks"],
                                "det_score": face["det_score"], "quality_metrics": q, "is_valid": ok})
                row += 1
            results.sort(key=lambda x: x["det_score"] * x["quality_metrics"].get("blur_score", 1000), reverse=True)
            out.append(results)
        return picked, out, crops

    def process_clip(self, frames, save: bool = True, save_partial: bool = False):
        """One capture session per clip.  ``frames``: a uint8 [n,H,W,3] RGB clip (array or tensor), or
        a list of clips for several cameras (one launch for all of them).  Returns the saved tracks
        of the clip, in track-id order, each ``{'track_id', 'crops' (uint8 [k,S,S,3], saved order:
        best first), 'crops_device', 'frames' (the clip's frame numbers, same order), 'qualities',
        'metadata' (the reference's metadata.json dict)}``; for a list of clips, one such list per
        clip.  ``save`` writes ``track_%03d/`` folders under ``output_dir`` (a list of clips:
        under ``output_dir/camera_%02d``); ``save_partial`` also keeps the tracks that did not reach
        ``target_frames`` (the reference's 's' key before quitting)."""
        import torch
        from . import _lib
        many = isinstance(frames, (list, tuple))
        clips = list(frames) if many else [frames]
        acc0 = self.accumulator
        per_clip = [self._faces_of_clip(c) for c in clips]
        faces = [f for _picked, per_frame, _crops in per_clip for fr in per_frame for f in fr]
        bbox = np.array([np.asarray(f["bbox"]).astype(int)[:4] for f in faces], dtype=np.int64).reshape(-1, 4)
        metrics = np.array([[f["det_score"]] + [f["quality_metrics"].get(k, 0) for k in METRIC_KEYS] for f in faces],
                           dtype=np.float64).reshape(-1, 5)
        valid = np.array([bool(f["is_valid"]) for f in faces], dtype=np.uint8)
        if not np.isfinite(metrics).all():
            raise ValueError("non-finite quality metrics (det_score, blur_score, yaw, pitch, roll)")
        if len(faces) and np.abs(bbox).max() > CAPTURE_COORD_MAX:
            raise NotImplementedError(f"a box coordinate beyond +-{CAPTURE_COORD_MAX}")
        frame_offsets = np.concatenate([[0], np.cumsum([len(fr) for _p, per_frame, _c in per_clip
                                                        for fr in per_frame])]).astype(np.int32)
        clip_offsets = np.concatenate([[0], np.cumsum([len(per_frame) for _p, per_frame, _c in per_clip])]
                                      ).astype(np.int32)
        if not hasattr(self, "_handle"):
            self._handle = _lib.Handle("ir_50", "adaface", self.device, max_batch=1)  # never finalised
        dev = self._handle.device
        track_id, quality, slot, info = self._handle.capture_tracks(
            torch.from_numpy(bbox.astype(np.int32)).to(dev), torch.from_numpy(metrics).to(dev),
            torch.from_numpy(valid).to(dev), frame_offsets, clip_offsets, self.tracker.max_disappeared,
            self.tracker.max_distance, acc0.target_frames, acc0.min_quality_score, save_partial)
        # the saved crops of every track, gathered on the device in (clip, track, slot) order
        track_id, quality, slot, info = (x.cpu().numpy() for x in (track_id, quality, slot, info))
        det_clip = np.repeat(np.arange(len(clips)), np.diff(frame_offsets[clip_offsets]))
        saved = np.flatnonzero(slot >= 0)
        order = saved[np.lexsort((slot[saved], track_id[saved], det_clip[saved]))]
        crops = torch.cat([c for _p, _f, c in per_clip]) if per_clip else None
        rows = np.array([f["crop_row"] for f in faces], dtype=np.int64)
        base = np.concatenate([[0], np.cumsum([len(c) for _p, _f, c in per_clip])])
        rows = rows + base[det_clip] if len(faces) else rows
        gathered = crops[torch.from_numpy(rows[order]).to(crops.device)] if len(order) else crops[:0]
        host = gathered.cpu().numpy()
        det_frame = np.repeat(np.arange(len(frame_offsets) - 1), np.diff(frame_offsets))
        # the reference's bookkeeping, per clip
        self.accumulators, self.total_tracks, results = [], [], []
        self.frame_count = int(sum(len(c) for c in clips))
        at = 0
        for c in range(len(clips)):
            acc = acc0 if not many else FrameAccumulator(acc0.target_frames, acc0.min_quality_score,
                                                         os.path.join(acc0.output_dir, f"camera_{c:02d}"),
                                                         verbose=acc0.verbose)
            if not many:
                acc.accumulated_frames.clear(), acc.completed_tracks.clear(), acc.metadata.clear()
            picked = per_clip[c][0]
            tracks = []
            mine = order[det_clip[order] == c]
            for tid in np.unique(track_id[mine]):
                dets = mine[track_id[mine] == tid]  # slot order
                k = len(dets)
                acc.accumulated_frames[int(tid)] = [
                    {"aligned_face": host[at + j], "quality_score": float(quality[i]),
                     "det_score": faces[i]["det_score"], "metrics": faces[i]["quality_metrics"],
                     "timestamp": datetime.now().isoformat()} for j, i in enumerate(dets)]
                acc.save_track(int(tid), write=save)
                tracks.append({"track_id": int(tid), "crops": host[at:at + k], "crops_device": gathered[at:at + k],
                               "frames": [picked[det_frame[i] - clip_offsets[c]] for i in dets],
                               "qualities": [float(quality[i]) for i in dets], "metadata": acc.metadata[int(tid)]})
                at += k
            self.accumulators.append(acc)
            self.total_tracks.append(int(info[c, 0]))
            results.append(tracks)
        self.tracker.next_track_id = self.total_tracks[0] + 1 if self.total_tracks else 1
        self.last_clip_info = info
        return results if many else results[0]

    def recognize_clip(self, frames, matcher, top_k: int = 3, save: bool = False, save_partial: bool = False):
        """``process_clip`` then ``FaceMatcher.match_tracks`` on the saved crops: ``(tracks,
        match_tracks' result per track)`` for a clip, or a list of such pairs for a list of clips."""
        many = isinstance(frames, (list, tuple))
        per_clip = self.process_clip(frames, save=save, save_partial=save_partial)
        per_clip = per_clip if many else [per_clip]
        names = [[t["metadata"]["files"] for t in tracks] for tracks in per_clip]
        flat = [list(t["crops"]) for tracks in per_clip for t in tracks]
        matched = matcher.match_tracks(flat, top_k=top_k, frame_names=[n for ns in names for n in ns])
        out, at = [], 0
        for tracks in per_clip:
            out.append((tracks, matched[at:at + len(tracks)]))
            at += len(tracks)
        return out if many else out[0]

    def save_summary(self):
        """:384-405: ``session_summary.json`` beside the track folders (one per clip's folder)."""
        summaries = []
        for acc, total in zip(self.accumulators, self.total_tracks):
            summary = {
                "session_end": datetime.now().isoformat(),
                "total_frames_processed": self.frame_count,
                "total_tracks": total,
                "completed_tracks": len(acc.completed_tracks),
                "tracks": acc.metadata,
            }
            summary_path = os.path.join(acc.output_dir, "session_summary.json")
            os.makedirs(acc.output_dir, exist_ok=True)
            with open(summary_path, "w") as f:
                json.dump(summary, f, indent=2)
            if self.verbose:
                print("\n" + "=" * 60)
                print("SESSION SUMMARY")
                print("=" * 60)
                print(f"Total tracks: {summary['total_tracks']}")
                print(f"Completed tracks: {summary['completed_tracks']}")
                print(f"Frames processed: {summary['total_frames_processed']}")
                print(f"Output directory: {acc.output_dir}")
                print(f"Summary saved to: {summary_path}")
                print("=" * 60 + "\n")
            summaries.append(summary)
        return summaries if len(summaries) != 1 else summaries[0]
