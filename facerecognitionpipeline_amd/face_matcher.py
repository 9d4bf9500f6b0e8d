"""``FaceMatcher`` — the reference's matcher (face_matcher.py:19-500) on the device.

``match_single_face`` is one embed + match unit (:52-58) and ``match_faces`` its batched form:
every crop of a frame (or every due track) in one ``fr_embed_match``.

The offline attendance flow (:60-146, :321-500) is mirrored too: ``match_track``,
``process_capture_directory``, ``_generate_summary`` / ``_print_summary`` and the two vote
functions ``_aggregate_matches`` / ``_get_best_candidate`` keep the reference's names,
arguments, dict keys and ``None`` cases.  Where the reference embeds and searches one frame at
a time, ``match_tracks`` runs all frames of all tracks through one ``match_faces`` pass and
decides every track in one ``fr_track_consensus`` launch on the top-k output while it is still
in HBM; ``_aggregate_matches`` / ``_get_best_candidate`` are the host statement of the same
vote (and serve tracks longer than the kernel's 1024 frames).

Out of scope: ``match_single_image`` (needs a loaded detector; ``FaceProcessor`` +
``match_faces`` cover it), ``_save_match_visualization`` (cv2 drawing) and the CLI ``main``.
"""
from __future__ import annotations

import json
import os
from collections import Counter
from datetime import datetime
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .face_embedder import FaceEmbedder
from .gallery_manager import GalleryManager, _slice_len, check_identity_aggregation

# include/frhip.h FR_TRACK_*
TRACK_RECOGNIZED, TRACK_FEW_FRAMES, TRACK_NO_CONSENSUS, TRACK_BELOW_THRESHOLD = 0, 1, 2, 3
TRACK_MAX_FRAMES = 1024
TRACK_STATUS_NAMES = ("recognized", "few_frames", "no_consensus", "below_threshold")
MIN_QUALITY = 0.55  # face_matcher.py:324 / :366
MIN_FRAMES = 3      # face_matcher.py:325


def track_consensus_host(keys: Sequence, scores: Sequence[float], min_quality: float = MIN_QUALITY,
                         min_frames: int = MIN_FRAMES, similarity_threshold: float = 0.5):
    """The vote of face_matcher.py:321-385 on one track's top-1 ``keys`` (student ids or gallery
    rows) and ``scores``; what ``fr_track_consensus`` computes per track.  Returns
    ``(status, winner_key, winner_count, pool_size, second_count, n_frames, quality_frames,
    confidence, ratio)``.  ``len(keys)`` must be >= 1."""
    scores = [float(s) for s in scores]
    quality = [i for i, s in enumerate(scores) if s >= min_quality]
    pool = quality or list(range(len(scores)))  # no quality frame: every frame (:367-370)
    ranked = Counter(keys[i] for i in pool).most_common(2)  # equal counts: first seen first
    winner, winner_count = ranked[0]
    second_count = ranked[1][1] if len(ranked) > 1 else 0
    ratio = winner_count / len(pool)
    consensus = ratio > 0.5
    if not consensus and second_count > 0:
        consensus = ratio > 0.4 and winner_count >= 2 * second_count
    confidence = float(np.mean([scores[i] for i in pool if keys[i] == winner]))
    if len(quality) < min_frames:
        status = TRACK_FEW_FRAMES
    elif not consensus:
        status = TRACK_NO_CONSENSUS
    elif confidence < similarity_threshold:
        status = TRACK_BELOW_THRESHOLD
    else:
        status = TRACK_RECOGNIZED
    return status, winner, winner_count, len(pool), second_count, len(scores), len(quality), confidence, ratio


class FaceMatcher:
    def __init__(self, gallery_path: Optional[str] = None, similarity_threshold: float = 0.5,
                 aggregation_method: str = "majority_vote", model_type: str = "adaface",
                 architecture: str = "ir_101", model_path: Optional[str] = None, device=None,
                 embedder: Optional[FaceEmbedder] = None, gallery: Optional[GalleryManager] = None,
                 verbose: bool = True, identity_aggregation: Optional[str] = None, identity_k: int = 3):
        """``identity_aggregation`` ('max' / 'mean' / 'topk'; ``identity_k`` is the top-k mean's k) makes
        every match score each student over all of its stored embeddings, as the evaluation notebook's
        ``identify_probe`` does, in place of the one template per student (None, the default):
        ``similarity_threshold`` then applies to that identity score.  (``aggregation_method`` is the
        reference's name for the track vote.)"""
        check_identity_aggregation(identity_aggregation, identity_k)
        self.identity_aggregation = identity_aggregation
        self.identity_k = int(identity_k)
        self.similarity_threshold = similarity_threshold
        self.aggregation_method = aggregation_method
        self.model_type = model_type
        self.architecture = architecture
        self.verbose = verbose  # the track methods print what the reference prints
        self.embedder = embedder or FaceEmbedder(architecture=architecture, model_path=model_path,
                                                 model_type=model_type, device=device)
        self.gallery = gallery or GalleryManager(gallery_path=gallery_path, device=self.embedder.device)
        self.gallery.attach_handle(self.embedder.model)

    def _print(self, *args, **kw) -> None:
        if self.verbose:
            print(*args, **kw)

    def _embed_match(self, rgb: torch.Tensor):
        """The ``launch`` of ``GalleryManager.match_resolved``: one library call from crops to top-k."""
        agg, agg_k = self.identity_aggregation, self.identity_k
        if agg is None:
            return lambda h, k, idx, score: h.embed_match(rgb, k, idx, score)
        return lambda h, k, idx, score: h.embed_match_identities(rgb, agg, agg_k, k, idx, score)

    def match_single_face(self, face_image: np.ndarray, top_k: int = 5) -> List[Tuple[str, str, float]]:
        if self.identity_aggregation is not None:
            return self.match_faces([face_image], top_k=top_k)[0]
        embedding = self.embedder.extract_embedding(face_image, normalize=True)
        return self.gallery.search(embedding, top_k=top_k)

    def match_faces(self, face_images: Sequence[np.ndarray], top_k: int = 5) -> List[List[Tuple[str, str, float]]]:
        """Batched match_single_face: one device embed+match for all crops."""
        if len(face_images) == 0:
            return []
        rgb = self.embedder.to_device_crops(list(face_images))  # validates; resizes non-112 crops
        return self.gallery.match_resolved(len(face_images), top_k, self._embed_match(rgb),
                                           self.identity_aggregation, self.identity_k)

    # -- tracks ----------------------------------------------------------------
    def _vote(self, frame_matches: List[Dict]):
        return track_consensus_host([m["student_id"] for m in frame_matches], [m["score"] for m in frame_matches],
                                    MIN_QUALITY, MIN_FRAMES, self.similarity_threshold)

    def _aggregate_matches(self, frame_matches: List[Dict], all_scores: Dict[str, List[float]]) -> Optional[Dict]:
        """face_matcher.py:321-363: the consensus winner of a track's frames, or None (fewer than
        3 frames scoring >= 0.55, no consensus, or a mean winner score below the threshold).
        ``all_scores`` is accepted and, as in the reference, not used."""
        if not frame_matches:
            return None
        status, winner, count, _pool, _second, n, _nq, confidence, ratio = self._vote(frame_matches)
        if status != TRACK_RECOGNIZED:
            return None
        name = next(m["name"] for m in frame_matches if m["student_id"] == winner)
        return {"student_id": winner, "name": name, "confidence": confidence, "consensus_strength": ratio,
                "num_quality_frames": count, "total_frames_evaluated": n}

    def _get_best_candidate(self, frame_matches: List[Dict], all_scores: Dict[str, List[float]]) -> Dict:
        """face_matcher.py:365-385: the most voted student of the quality frames (of all frames when
        there is none) and the mean of its scores there."""
        if not frame_matches:
            raise IndexError("no frame matches")  # the reference's most_common(1)[0] on no votes
        _status, winner, count, _pool, _second, _n, _nq, confidence, _ratio = self._vote(frame_matches)
        name = next(m["name"] for m in frame_matches if m["student_id"] == winner)
        return {"student_id": winner, "name": name, "confidence": confidence, "num_quality_frames": count}

    def match_tracks(self, tracks: Sequence[Sequence[np.ndarray]], top_k: int = 3,
                     frame_names: Optional[Sequence[Sequence[str]]] = None) -> List[Optional[Dict]]:
        """``match_track`` without the files, for many tracks at once: ``tracks[t]`` are the RGB
        crops of track t.  All frames of all tracks go through one ``match_faces`` pass and one
        ``fr_track_consensus`` launch.  Per track: None (no frames, or an empty gallery), or
        ``match_track``'s dict without ``track_id`` / ``metadata`` / ``timestamp``, plus
        ``'consensus'``: the vote's record (``status`` says which of the reference's three
        'below_threshold' cases applied).  ``frame_names[t][i]`` is frame i's ``'frame'`` entry
        (default: its index as ``'%06d'``)."""
        lengths = [len(t) for t in tracks]
        out: List[Optional[Dict]] = [None] * len(lengths)
        # tracks the kernel takes first, in order; over-long ones behind them, decided on the host
        order = ([t for t, n in enumerate(lengths) if 0 < n <= TRACK_MAX_FRAMES]
                 + [t for t, n in enumerate(lengths) if n > TRACK_MAX_FRAMES])
        if not order:
            return out
        n_dev = sum(1 for t in order if lengths[t] <= TRACK_MAX_FRAMES)
        offsets = np.concatenate([[0], np.cumsum([lengths[t] for t in order])]).astype(np.int64)
        frames = [f for t in order for f in tracks[t]]
        rgb = self.embedder.to_device_crops(frames)  # validates; resizes non-112 crops
        thr = float(self.similarity_threshold)

        def consensus(h, idx, score):
            n_rows = int(offsets[n_dev])
            if n_dev == 0:
                return None
            rec_i, rec_d = h.track_consensus(idx[:n_rows], score[:n_rows], offsets[:n_dev + 1], MIN_QUALITY,
                                             MIN_FRAMES, thr)
            return rec_i.cpu().numpy(), rec_d.cpu().numpy(), idx[:n_rows, 0].cpu().numpy()

        # (with identity_aggregation idx holds identity indices, one per student like the template
        # rows, so the vote and the id resolution read them the same way)
        matches, dev = self.gallery.match_resolved_with(len(frames), top_k, self._embed_match(rgb), consensus,
                                                        self.identity_aggregation, self.identity_k)
        if not matches or not matches[0]:  # empty gallery (or top_k selecting nothing): no valid matches
            return out
        for j, t in enumerate(order):
            lo, hi = int(offsets[j]), int(offsets[j + 1])
            names = frame_names[t] if frame_names is not None else [f"{i:06d}" for i in range(hi - lo)]
            fm = [{"frame": names[i], "student_id": m[0][0], "name": m[0][1], "score": float(m[0][2]),
                   "top_k_matches": [{"student_id": sid, "name": n, "score": float(s)} for sid, n, s in m]}
                  for i, m in enumerate(matches[lo:hi])]
            if j < n_dev:
                ri, rd, row0 = dev[0][j], dev[1][j], dev[2][lo:hi]
                first = fm[int(np.flatnonzero(row0 == ri[1])[0])]  # rows and ids are one-to-one
                rec = (int(ri[0]), first["student_id"], int(ri[2]), int(ri[3]), int(ri[4]), int(ri[5]), int(ri[6]),
                       float(rd[0]), float(rd[1]))
            else:
                rec = self._vote(fm)
                first = next(m for m in fm if m["student_id"] == rec[1])
            status, winner, count, pool, second, n, nq, confidence, ratio = rec
            record = {"status": TRACK_STATUS_NAMES[status], "consensus_strength": ratio, "winner_frames": count,
                      "pool_frames": pool, "second_frames": second, "quality_frames": nq,
                      "total_frames_evaluated": n}
            if status == TRACK_RECOGNIZED:
                out[t] = {"recognized": True, "student_id": winner, "name": first["name"], "confidence": confidence,
                          "method": self.aggregation_method, "num_frames": len(fm), "frame_matches": fm,
                          "consensus": record}
            else:
                out[t] = {"recognized": False, "reason": "below_threshold",
                          "best_candidate": {"student_id": winner, "name": first["name"], "confidence": confidence,
                                             "num_quality_frames": count},
                          "frame_matches": fm, "consensus": record}
        return out

    def _read_track(self, track_dir: str):
        """(metadata, frame names, RGB frames) of a ``track_XXXX`` folder, or None where the
        reference's match_track returns None before matching (:64-75)."""
        from .face_recognition import load_image_rgb
        track_id = os.path.basename(track_dir)
        metadata_path = os.path.join(track_dir, "metadata.json")
        if not os.path.exists(metadata_path):
            self._print(f"No metadata found for {track_id}")
            return None
        with open(metadata_path, "r") as f:
            metadata = json.load(f)
        face_files = sorted(f for f in os.listdir(track_dir) if f.endswith(".jpg"))
        if len(face_files) == 0:
            self._print(f"No face images found in {track_id}")
            return None
        self._print(f"\nProcessing {track_id}: {len(face_files)} frames")
        names, frames = [], []
        for face_file in face_files:
            img = load_image_rgb(os.path.join(track_dir, face_file))
            if img is None:  # cv2.imread returned None: the frame is skipped (:86-87)
                continue
            names.append(face_file)
            frames.append(img)
        return metadata, names, frames

    def _track_result(self, track_dir: str, loaded, matched: Optional[Dict]) -> Optional[Dict]:
        track_id = os.path.basename(track_dir)
        if matched is None:
            self._print("No valid matches found")
            return None
        metadata = loaded[0]
        if not matched["recognized"]:
            best_candidate = matched["best_candidate"]
            self._print(f"Below threshold - Best candidate: {best_candidate['name']} "
                        f"({best_candidate['student_id']}) - confidence: {best_candidate['confidence']:.3f}")
            return {"track_id": track_id, "recognized": False, "reason": "below_threshold",
                    "best_candidate": best_candidate, "frame_matches": matched["frame_matches"],
                    "metadata": metadata, "timestamp": datetime.now().isoformat()}
        self._print(f"  ✓ Identified: {matched['name']} ({matched['student_id']}) - "
                    f"confidence: {matched['confidence']:.3f}")
        return {"track_id": track_id, "recognized": True, "student_id": matched["student_id"],
                "name": matched["name"], "confidence": matched["confidence"], "method": matched["method"],
                "num_frames": matched["num_frames"], "frame_matches": matched["frame_matches"],
                "metadata": metadata, "timestamp": datetime.now().isoformat()}

    def _match_track_dirs(self, track_dirs: Sequence[str], top_k: int) -> List[Optional[Dict]]:
        loaded = [self._read_track(d) for d in track_dirs]
        matched = self.match_tracks([x[2] if x else [] for x in loaded], top_k=top_k,
                                    frame_names=[x[1] if x else [] for x in loaded])
        return [self._track_result(d, x, m) if x else None for d, x, m in zip(track_dirs, loaded, matched)]

    def match_track(self, track_dir: str, top_k: int = 3) -> Optional[Dict]:
        """face_matcher.py:60-146 on one ``track_XXXX`` folder (``metadata.json`` + ``*.jpg`` crops):
        the reference's dict for a recognized track, its ``recognized=False,
        reason='below_threshold', best_candidate=...`` dict otherwise, or None (no metadata, no
        readable frame, empty gallery)."""
        return self._match_track_dirs([track_dir], top_k)[0]

    def process_capture_directory(self, capture_dir: str, save_results: bool = True) -> Dict:
        """face_matcher.py:387-444: every ``track_*`` folder of ``capture_dir`` (one
        ``match_tracks`` pass for all of them), ``recognition_result.json`` per track and
        ``<model_type>_<architecture>_results/recognition_summary.json``."""
        if not os.path.exists(capture_dir):
            raise ValueError(f"Capture directory not found: {capture_dir}")
        self._print("\n" + "=" * 60)
        self._print("PROCESSING CAMERA CAPTURES")
        self._print(f"Directory: {capture_dir}")
        self._print("=" * 60)
        track_dirs = [os.path.join(capture_dir, item) for item in sorted(os.listdir(capture_dir))
                      if item.startswith("track_") and os.path.isdir(os.path.join(capture_dir, item))]
        if len(track_dirs) == 0:
            self._print("No track directories found!")
            return {"error": "no_tracks"}
        self._print(f"Found {len(track_dirs)} tracks to process\n")
        results = []
        recognized_count = unrecognized_count = 0
        for track_dir, result in zip(track_dirs, self._match_track_dirs(track_dirs, top_k=3)):
            if result is None:
                continue
            results.append(result)
            if result["recognized"]:
                recognized_count += 1
            else:
                unrecognized_count += 1
            if save_results:
                with open(os.path.join(track_dir, "recognition_result.json"), "w") as f:
                    json.dump(result, f, indent=2)
        summary = self._generate_summary(results, recognized_count, unrecognized_count)
        if save_results:
            results_dir = os.path.join(capture_dir, f"{self.model_type}_{self.architecture}_results")
            os.makedirs(results_dir, exist_ok=True)
            summary_path = os.path.join(results_dir, "recognition_summary.json")
            with open(summary_path, "w") as f:
                json.dump(summary, f, indent=2)
            self._print(f"\nSummary saved to: {summary_path}")
        self._print_summary(summary)
        return summary

    def _generate_summary(self, results: List[Dict], recognized: int, unrecognized: int) -> Dict:
        """face_matcher.py:446-477."""
        student_counts: Counter = Counter()
        for result in results:
            if result["recognized"]:
                student_counts[result["name"]] += 1
        confidences = [r["confidence"] for r in results if r["recognized"]]
        avg_confidence = np.mean(confidences) if confidences else 0
        below_threshold = [r["best_candidate"] for r in results if not r["recognized"] and "best_candidate" in r]
        return {
            "total_tracks": len(results),
            "recognized": recognized,
            "unrecognized": unrecognized,
            "recognition_rate": recognized / len(results) * 100 if results else 0,
            "avg_confidence": float(avg_confidence),
            "student_appearances": dict(student_counts.most_common()),
            "below_threshold_candidates": below_threshold,
            "unique_students": len(student_counts),
            "timestamp": datetime.now().isoformat(),
            "settings": {"similarity_threshold": self.similarity_threshold,
                         "aggregation_method": self.aggregation_method},
        }

    def _print_summary(self, summary: Dict) -> None:
        """face_matcher.py:479-500."""
        self._print("\n" + "=" * 60)
        self._print("RECOGNITION SUMMARY")
        self._print("=" * 60)
        self._print(f"Total tracks: {summary['total_tracks']}")
        self._print(f"Recognized: {summary['recognized']} ({summary['recognition_rate']:.1f}%)")
        self._print(f"Unrecognized: {summary['unrecognized']}")
        self._print(f"Average confidence: {summary['avg_confidence']:.3f}")
        self._print(f"Unique students detected: {summary['unique_students']}")
        if summary["student_appearances"]:
            self._print("\nStudent appearances:")
            for name, count in summary["student_appearances"].items():
                self._print(f"  • {name}: {count} track(s)")
        if summary.get("below_threshold_candidates"):
            self._print("\nBelow threshold (not recognized):")
            for candidate in summary["below_threshold_candidates"]:
                self._print(f"  • {candidate['name']}: confidence {candidate['confidence']:.3f} "
                            f"(needed {self.similarity_threshold})")
        self._print("=" * 60 + "\n")
