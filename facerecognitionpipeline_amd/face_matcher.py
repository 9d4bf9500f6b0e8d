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

The photograph flow (:148-319, ``--single_image``) is ``match_single_image`` and its batched form
``match_images``: detect, align and blur over all photographs in one pass, the crops gathered into
result order on the device, one embed + match launch, and every face decided by
``fr_photo_rollcall`` on the resident top-k output (``photo_rollcall_host`` is the host statement
of that rule).  ``exclusive=True`` is not in the reference: a student is then given to at most one
face of a photograph.  ``_save_match_visualization`` keeps the reference's path rule and colours and
draws with PIL, and ``main`` takes the reference's arguments.

Out of scope: ``visualize_detections`` (matplotlib).
"""
from __future__ import annotations

import argparse
import json
import os
from collections import Counter
from datetime import datetime
from pathlib import Path
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
# include/frhip.h FR_ROLLCALL_* / FR_FACE_*
ROLLCALL_INDEPENDENT, ROLLCALL_EXCLUSIVE = 0, 1
FACE_RECOGNIZED, FACE_CANDIDATE, FACE_DISPLACED = 0, 1, 2
ROLLCALL_MAX_FACES = 1024
SCRIPT_DIR = Path(__file__).resolve().parent
# face_matcher.py:160-174: the processor match_single_image builds
PHOTO_PROCESSOR_CONFIG = {
    "output_size": 112, "det_size": (640, 640), "det_thresh": 0.5,
    "quality_filter_config": {"min_det_score": 0.5, "min_face_size": 40, "max_yaw": 60, "max_pitch": 45,
                              "max_roll": 45, "check_blur": True, "blur_threshold": 50},
    "providers": ["CUDAExecutionProvider", "CPUExecutionProvider"],
}


def photo_rollcall_host(idx, score, offsets, similarity_threshold: float = 0.5, mode: int = ROLLCALL_INDEPENDENT):
    """What ``fr_photo_rollcall`` computes (include/frhip.h), stated as a sort and a scan: ``idx`` int32
    / ``score`` float32 [total,k] top-k rows, photograph p = faces [offsets[p], offsets[p+1]) (any
    number of faces) -> (out_face int32 [total,4] = status, row, column, 0; out_score float32 [total];
    out_image int32 [P,4] = faces, recognized, candidates, displaced)."""
    if mode not in (ROLLCALL_INDEPENDENT, ROLLCALL_EXCLUSIVE):
        raise ValueError("mode must be ROLLCALL_INDEPENDENT or ROLLCALL_EXCLUSIVE")
    idx = np.asarray(idx, np.int32)
    score = np.asarray(score, np.float32)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    total = idx.shape[0]
    out_face = np.zeros((total, 4), np.int32)
    out_score = np.zeros(total, np.float32)
    out_image = np.zeros((len(offsets) - 1, 4), np.int32)
    with np.errstate(invalid="ignore"):
        claim = score.astype(np.float64) >= float(similarity_threshold)  # never true for a NaN
    for p, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        granted: Dict[int, int] = {}  # face -> column
        if mode == ROLLCALL_EXCLUSIVE:
            f, c = np.nonzero(claim[lo:hi])
            s = score[lo:hi][f, c]
            held = set()
            # score descending (as f32 values), then face, then column ascending
            for j in np.lexsort((c, f, -s)):
                face, row = int(f[j]), int(idx[lo + f[j], c[j]])
                if face not in granted and row not in held:
                    granted[face] = int(c[j])
                    held.add(row)
        for face in range(int(hi - lo)):
            at = int(lo) + face
            if mode == ROLLCALL_EXCLUSIVE:
                col = granted.get(face, 0)
                status = (FACE_RECOGNIZED if face in granted else
                          FACE_DISPLACED if claim[at, 0] else FACE_CANDIDATE)
            else:
                col, status = 0, (FACE_RECOGNIZED if claim[at, 0] else FACE_CANDIDATE)
            out_face[at] = (status, idx[at, col], col, 0)
            out_score[at] = score[at, col]
            out_image[p, 1 + status] += 1
        out_image[p, 0] = hi - lo
    return out_face, out_score, out_image


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

    # -- photographs -----------------------------------------------------------
    processor = None  # the FaceProcessor of match_single_image / match_images, kept between calls

    def _photo_processor(self):
        if self.processor is None:
            from .face_recognition import FaceProcessor
            self.processor = FaceProcessor(**PHOTO_PROCESSOR_CONFIG, device=self.embedder.device)
        return self.processor

    def match_single_image(self, image_path: str, top_k: int = 5, save_visualization: bool = True,
                           processor=None, exclusive: bool = False, device_chain: bool = False) -> Dict:
        """face_matcher.py:148-271: every face of the photograph at ``image_path`` (``return_all``: the
        quality gate is reported, not applied) against the gallery -> the reference's dict.
        ``processor`` replaces the ``FaceProcessor`` of the reference's configuration (built on first
        use otherwise) and is kept for later calls.  ``exclusive`` and ``device_chain``: see
        :meth:`match_images`, of which this is the one-path case."""
        if not isinstance(device_chain, bool):
            raise ValueError("device_chain must be True or False")
        if processor is not None:
            self.processor = processor
        if not os.path.exists(image_path):
            self._print(f"\n{'=' * 60}")
            self._print(f"MATCHING IMAGE: {image_path}")
            self._print(f"{'=' * 60}")
            raise ValueError(f"Image not found: {image_path}")
        return self.match_images([image_path], top_k=top_k, exclusive=exclusive,
                                 save_visualization=save_visualization, device_chain=device_chain)[0]

    def match_images(self, images, top_k: int = 5, exclusive: bool = False, save_visualization: bool = False,
                     errors: str = "raise", device_chain: bool = False) -> List:
        """``match_single_image`` for a sequence of photographs of different sizes -- paths or arrays,
        as ``FaceProcessor.process_images`` takes them (and its ``errors``) -- in one pass: one detect
        call, one align launch at the processor's size and one blur call over all photographs; the
        crops stay on the device, are gathered there into result order (``process_numpy``'s: det_score
        x blur_score descending, which ``face_index`` counts) and go through one ``embed_match`` /
        ``embed_match_identities`` launch; ``fr_photo_rollcall`` decides every face on the top-k output
        before it is copied out.  Returns one ``match_single_image`` dict per item (``image_path`` is
        None for an array; an array is not visualised).

        ``exclusive=False`` is the reference's rule: a face is recognised if its top-1 score reaches
        the threshold, so two faces of a photograph may both come out as one student.
        ``exclusive=True`` lets a student be held by one face of a photograph only (the rule of
        ``fr_photo_rollcall``'s FR_ROLLCALL_EXCLUSIVE): a recognised face also carries ``match_rank``,
        the 1-based rank among its ``top_matches`` that it was given, and a face that lost its top-1 and
        every other match above the threshold has ``recognized: False``, its top-1 as
        ``best_candidate`` and ``reason: 'claimed_by_other_face'``.

        ``device_chain=True`` runs the photographs through ``device_chain_images`` (the processor must
        hold the GPU ``FaceDetector``: TypeError otherwise): detections stay in HBM through the fit, the
        warp, the blur score and the quality gate, the gate's ``rows`` gather the crops into result
        order on the device and its ``frame_offsets`` are the roll call's offsets, so the only copies
        to the host are one packed copy of the per-slot outputs per block of the detector's
        ``max_frames`` photographs and the top-k results.  The same dicts as with ``False`` (metrics as
        ``FaceProcessor.process_frames`` states); a detection whose similarity fit fails is listed with
        ``is_valid: False`` where the host path raises."""
        if not isinstance(device_chain, bool):
            raise ValueError("device_chain must be True or False")
        processor = self._photo_processor()
        if device_chain:
            if not hasattr(getattr(processor.detector, "model", None), "detect_images_device"):
                raise TypeError("device_chain=True runs the GPU FaceDetector (detect_images_device); the "
                                "processor's detector has none")
            out, items = processor._usable_items(images, errors)
            # the live crops in result order, image after image: already the embedder's order
            per_image, crops = processor._chain_images([image for _slot, image in items], True) if items else (
                [], None)
            order = list(range(sum(len(r) for r in per_image)))
        else:
            out, items, faces, crops, blur = processor._detect_align_images(images, errors)
            per_image, order, at = [], [], 0
            for (_slot, _image), fs in zip(items, faces):
                # the gate, sort and dicts of process_numpy, with a crop's position in place of the crop
                res = processor._gate(fs, np.arange(at, at + len(fs)),
                                      None if blur is None else blur[at:at + len(fs)], True) if fs else []
                per_image.append(res)
                order.extend(int(r["aligned_face"]) for r in res)
                at += len(fs)
        n = len(order)
        offsets = np.concatenate([[0], np.cumsum([len(r) for r in per_image])]).astype(np.int64)
        thr = float(self.similarity_threshold)
        mode = ROLLCALL_EXCLUSIVE if exclusive else ROLLCALL_INDEPENDENT
        matches, decided = [], None
        if n:
            rgb = crops.to(self.embedder.device)
            if order != list(range(n)):
                rgb = rgb[torch.as_tensor(order, dtype=torch.int64, device=rgb.device)]
            if tuple(rgb.shape[1:3]) != (112, 112):  # a processor of another output_size
                resized = torch.empty((n, 112, 112, 3), dtype=torch.uint8, device=rgb.device)
                self.embedder.model.resize_crops(rgb.contiguous(), resized)
                rgb = resized
            rgb = rgb.contiguous()
            on_device = max(len(r) for r in per_image) <= ROLLCALL_MAX_FACES

            def rollcall(h, idx, score):
                if not on_device:
                    return None
                face, fscore, _image = h.photo_rollcall(idx, score, offsets, thr, mode)
                return face.cpu().numpy(), fscore.cpu().numpy()

            matches, decided = self.gallery.match_resolved_with(n, top_k, self._embed_match(rgb), rollcall,
                                                                self.identity_aggregation, self.identity_k)
            if decided is None and matches and matches[0]:
                # a photograph past the kernel's 1024 faces: the host statement, a student's id as its row
                key: Dict[str, int] = {}
                rows = np.array([[key.setdefault(sid, len(key)) for sid, _n, _s in m] for m in matches], np.int32)
                scores = np.array([[s for _sid, _n, s in m] for m in matches], np.float32)
                decided = photo_rollcall_host(rows, scores, offsets, thr, mode)[:2]
        for j, ((slot, _image), res) in enumerate(zip(items, per_image)):
            item = images[slot]
            path = os.fspath(item) if isinstance(item, (str, bytes)) or hasattr(item, "__fspath__") else None
            lo = int(offsets[j])
            out[slot] = self._photo_result(path, res, matches[lo:lo + len(res)],
                                           None if decided is None else decided[0][lo:lo + len(res)],
                                           top_k, exclusive, save_visualization and path is not None)
        return out

    def _photo_result(self, image_path, faces: List[Dict], results: List, decided, top_k: int, exclusive: bool,
                      save_visualization: bool) -> Dict:
        """The dict and the printing of face_matcher.py:152-271 for one photograph: ``faces`` in
        result order, ``results[i]`` the resolved top-k of face i, ``decided[i]`` its roll-call record
        (status, row, column, 0)."""
        self._print(f"\n{'=' * 60}")
        self._print(f"MATCHING IMAGE: {image_path}")
        self._print(f"{'=' * 60}")
        if len(faces) == 0:
            self._print("No faces detected in image")
            return {"image_path": image_path, "num_faces": 0, "matches": [], "timestamp": datetime.now().isoformat()}
        self._print(f"Detected {len(faces)} face(s)")
        matches = []
        for i, (face, res) in enumerate(zip(faces, results)):
            self._print(f"\nFace {i + 1}:")
            self._print(f"  Detection score: {face['det_score']:.3f}")
            self._print(f"  Valid: {face['is_valid']}")
            if face["quality_metrics"].get("blur_score"):
                self._print(f"  Blur score: {face['quality_metrics']['blur_score']:.0f}")
            if len(res) == 0:
                self._print("  No matches found in gallery")
                matches.append({"face_index": i, "bbox": face["bbox"].tolist(), "recognized": False,
                                "reason": "no_gallery_matches", "quality_metrics": face["quality_metrics"]})
                continue
            status, _row, col, _pad = (int(v) for v in decided[i])
            recognized = status == FACE_RECOGNIZED
            student_id, name, score = res[col]
            if recognized:
                self._print(f"  ✓ Recognized: {name} ({student_id}) - confidence: {score:.3f}")
            elif status == FACE_DISPLACED:
                self._print(f"  ⚠ Claimed by another face: {name} ({student_id}) - confidence: {score:.3f}")
            else:
                self._print(f"  ⚠ Below threshold: {name} ({student_id}) - confidence: {score:.3f} "
                            f"(threshold: {self.similarity_threshold})")
            m = {"face_index": i, "bbox": face["bbox"].tolist(), "recognized": recognized,
                 "confidence": float(score), "quality_metrics": face["quality_metrics"],
                 "top_matches": [{"student_id": sid, "name": n, "score": float(s), "rank": rank + 1}
                                 for rank, (sid, n, s) in enumerate(res)]}
            if recognized:
                m["student_id"] = student_id
                m["name"] = name
                if exclusive:
                    m["match_rank"] = col + 1
            else:
                m["best_candidate"] = {"student_id": student_id, "name": name, "confidence": float(score)}
                if status == FACE_DISPLACED:
                    m["reason"] = "claimed_by_other_face"
            matches.append(m)
            self._print(f"  Top {min(top_k, len(res))} matches:")
            for rank, (sid, n, s) in enumerate(res[:top_k], 1):
                marker = "→" if rank == 1 else " "
                self._print(f"    {marker} {rank}. {n} ({sid}): {s:.3f}")
        if save_visualization:
            output_path = self._save_match_visualization(image_path, faces, matches)
            self._print(f"\nVisualization saved to: {output_path}")
        result = {"image_path": image_path, "num_faces": len(faces),
                  "num_recognized": sum(1 for m in matches if m.get("recognized", False)), "matches": matches,
                  "threshold": self.similarity_threshold, "timestamp": datetime.now().isoformat()}
        self._print(f"\n{'=' * 60}")
        self._print(f"Summary: {result['num_recognized']}/{result['num_faces']} faces recognized")
        self._print(f"{'=' * 60}\n")
        return result

    def _save_match_visualization(self, image_path: str, faces: List[Dict], matches: List[Dict]) -> str:
        """face_matcher.py:273-319: a box and two label lines per face -- green for a recognised face,
        (255, 165, 0) for a candidate, red otherwise -- written to
        ``<gallery stem>_match_results/matched_<filename>`` beside the image.  Drawn with PIL (cv2 is
        not a dependency): the path, the colours, the 3 px box and the label's place above it are the
        reference's; the glyphs are PIL's default font, not cv2's Hershey text, so pixel parity of the
        labels is not pinned."""
        from PIL import Image, ImageDraw, ImageFont
        from .face_recognition import load_image_rgb
        rgb = load_image_rgb(image_path)
        if rgb is None:
            raise ValueError(f"Could not load image: {image_path}")
        image = Image.fromarray(rgb, "RGB")
        draw = ImageDraw.Draw(image)
        font = ImageFont.load_default(size=22)  # about FONT_HERSHEY_SIMPLEX at scale 0.8
        for face, match in zip(faces, matches):
            x1, y1, x2, y2 = (int(v) for v in face["bbox"])
            if match.get("recognized", False):
                color = (0, 255, 0)
                label = f"{match['name']}\n{match['confidence']:.3f}"
            elif "best_candidate" in match:
                color = (255, 165, 0)
                cand = match["best_candidate"]
                label = f"{cand['name']}?\n{cand['confidence']:.3f}"
            else:
                color = (255, 0, 0)
                label = "Unknown"
            # cv2.rectangle's thickness 3 is centred on the box: one pixel to either side
            draw.rectangle([min(x1, x2) - 1, min(y1, y2) - 1, max(x1, x2) + 1, max(y1, y2) + 1], outline=color, width=3)
            y_offset = y1 - 10
            for line in reversed(label.split("\n")):
                left, top, right, bottom = draw.textbbox((0, 0), line, font=font)
                w, h = right - left, bottom - top
                y_offset -= h + 5
                draw.rectangle([x1, y_offset, x1 + w, y_offset + h + 5], fill=color)
                draw.text((x1 - left, y_offset - top + 2), line, fill=(0, 0, 0), font=font)
        gallery_name = Path(self.gallery.gallery_path).stem
        output_dir = os.path.join(os.path.dirname(image_path), f"{gallery_name}_match_results")
        os.makedirs(output_dir, exist_ok=True)
        output_path = os.path.join(output_dir, f"matched_{os.path.basename(image_path)}")
        image.save(output_path)
        return output_path

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


def main(argv: Optional[Sequence[str]] = None):
    """face_matcher.py:503-589, with the reference's arguments.  ``--single_image`` matches only the
    image (the reference runs the capture directory first, by mistake)."""
    parser = argparse.ArgumentParser(description="Match detected faces against student gallery")
    parser.add_argument("--capture_dir", type=str, default=str(SCRIPT_DIR / "output" / "camera_captures"),
                        help="Directory containing camera capture tracks")
    parser.add_argument("--gallery_path", type=str, default=str(SCRIPT_DIR / "gallery" / "students.pkl"),
                        help="Path to student gallery database")
    parser.add_argument("--threshold", type=float, default=0.35, help="Similarity threshold for positive match (0-1)")
    parser.add_argument("--aggregation", type=str, default="consensus",
                        choices=["consensus", "majority_vote", "avg_similarity", "max_similarity"],
                        help="Method to aggregate multi-frame matches")
    parser.add_argument("--no_save", action="store_true", help="Do not save recognition results to files")
    parser.add_argument("--single_image", type=str, default=None,
                        help="Path to single image to match (instead of processing capture directory)")
    parser.add_argument("--top_k", type=int, default=5, help="Number of top matches to show per face")
    parser.add_argument("--model_type", type=str, default="adaface", choices=["adaface", "arcface"],
                        help="Type of face recognition model to use")
    parser.add_argument("--architecture", type=str, default="ir_101", choices=["ir_50", "ir_101"],
                        help="Model architecture (ir_50 or ir_101)")
    args = parser.parse_args(argv)
    matcher = FaceMatcher(gallery_path=args.gallery_path, similarity_threshold=args.threshold,
                          aggregation_method=args.aggregation, model_type=args.model_type,
                          architecture=args.architecture)
    if args.single_image:
        return matcher.match_single_image(image_path=args.single_image, top_k=args.top_k, save_visualization=True)
    return matcher.process_capture_directory(capture_dir=args.capture_dir, save_results=not args.no_save)


if __name__ == "__main__":
    main()
