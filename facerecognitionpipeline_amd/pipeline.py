"""Batched frame-level recognition: the serving caller of the hot path.

The reference server recognises one face per request at batch 1 with a PNG
round trip in between (``face_recognition_server.py:314-347``, ``:586-739``).
Here one call takes a frame and its detections and runs, on the GPU, with the
frame uploaded once:

    align all faces (fr_align_faces)  ->  blur scores (fr_blur_scores)  ->
    quality gate (host scalars, face_recognition.py:123-158)  ->
    embed + match every valid face in one fr_embed_match  ->  top-k per face

Detections come from any detector with the reference ``FaceDetector.detect``
contract (``face_recognition.py:31-48``), the GPU SCRFD ``FaceDetector`` included.
``recognize_frames`` starts from the frames instead and keeps the whole chain on the
device: detect, align and blur write device buffers (fr_detect_device, fr_align_device,
fr_blur_scores_device), and a batch of frames crosses to the host once, for the gate.
``MatchBatcher`` batches concurrent single-face requests the same way.
"""
from __future__ import annotations

import queue
import threading
import time
from concurrent.futures import Future
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .face_embedder import FaceEmbedder, as_uint8_crop
from .face_recognition import FaceAligner, FaceDetector, FaceQualityFilter
from .gallery_manager import GalleryManager, _slice_len


class RecognitionPipeline:
    def __init__(self, embedder: FaceEmbedder, gallery: GalleryManager,
                 quality_filter_config: Optional[Dict] = None, similarity_threshold: float = 0.4,
                 detector: Optional[FaceDetector] = None):
        self.embedder = embedder
        self.detector = detector  # recognize_frames builds one on first use when None
        self.gallery = gallery
        self.gallery.attach_handle(embedder.model)
        dev = embedder.device
        self.aligner = FaceAligner(output_size=112, device=dev)
        self.quality = FaceQualityFilter(**(quality_filter_config or {}), device=dev)
        self.similarity_threshold = similarity_threshold

    def recognize(self, frame_rgb, detections: Sequence[Dict], top_k: int = 3) -> List[Dict]:
        """frame: uint8 [H,W,3] RGB (host array or device tensor); detections: reference dicts.

        Returns one dict per detection: quality metrics, ``is_valid`` and, for valid
        faces, ``matches`` = [(student_id, name, score)] and ``recognized`` (top-1
        score >= similarity_threshold, face_recognition_server.py:983-986).
        """
        dev = self.embedder.device
        if len(detections) == 0:
            return []
        frame = frame_rgb if isinstance(frame_rgb, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(frame_rgb, dtype=np.uint8))
        frame = frame.to(dev).contiguous()
        crops = self.aligner.align_batch(frame, np.stack([np.asarray(d["landmarks"], np.float32)
                                                          for d in detections]))
        blur = self.quality.compute_blur_scores(crops) if self.quality.check_blur else None
        out, valid = [], []
        for i, d in enumerate(detections):
            ok, q = self.quality.is_valid(d, None, None if blur is None else float(blur[i]))
            out.append({"bbox": d.get("bbox"), "det_score": d["det_score"], "quality_metrics": q,
                        "is_valid": ok, "matches": [], "recognized": False})
            if ok:
                valid.append(i)
        if not valid:
            return out
        sel = crops[torch.tensor(valid, device=dev)].contiguous()
        res = self.gallery.match_resolved(len(valid), top_k, lambda h, k, idx, score: h.embed_match(sel, k, idx, score))
        for row, i in enumerate(valid):
            m = res[row]
            out[i]["matches"] = m
            out[i]["recognized"] = bool(m) and m[0][2] >= self.similarity_threshold
        return out

    def recognize_frames(self, frames, top_k: int = 3, max_faces: Optional[int] = None,
                         gate: str = "host") -> List[List[Dict]]:
        """``recognize`` for a batch of frames, detection included: uint8 [n,H,W,3] RGB frames of one
        size (host array or device tensor) -> one list per frame of the dicts ``recognize(frame,
        detections)`` returns for the GPU detector's detections of that frame.

        detect_device -> align_device -> blur_scores_device run back to back on the device with
        ``max_faces`` slots per frame (default: the detector's ``max_faces``; crops of every slot are
        held, n * max_faces * 37.6 kB); then ONE copy brings dets, counts, ok and the blur scores to the
        host for the quality gate, and the valid crops are gathered on the device for one
        ``embed_match``.  A frame over the detector's 4096-candidate limit raises the
        ``NotImplementedError`` that ``FaceDetector.detect`` raises for it; a detection whose
        similarity fit fails (where ``recognize`` raises) comes back ``is_valid: False``.

        ``gate="device"`` runs the quality gate on the device as well (``fr_quality_gate_device``): the
        one copy then brings the gate's per-slot outputs and the number of valid faces, the valid
        crops are gathered through the gate's ``valid_slots`` without a host-built index, and the
        dicts are rebuilt with ``metrics_from_gate``.  The same faces, ids and flags; yaw and roll as
        ``quality_gate_host`` states them (within 1e-4 degrees of the host gate's); the valid crops
        are embedded in the gate's order (per frame by descending det_score x blur_score), another
        batch order, so scores agree within 1e-6."""
        if gate not in ("host", "device"):
            raise ValueError('gate must be "host" or "device"')
        dev = self.embedder.device
        if self.detector is None:
            self.detector = FaceDetector(device=dev)
        det = self.detector
        if det.device != dev:
            raise ValueError(f"the detector is on {det.device}, the embedder on {dev}")
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8))
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("expected uint8 [n,H,W,3] RGB frames")
        n = t.shape[0]
        if n == 0:
            return []
        t = t.to(dev).contiguous()
        F = det.max_faces if max_faces is None else int(max_faces)
        S = self.aligner.output_size
        dets, counts = det.model.detect_device(t, det.det_thresh, F)
        crops, _, ok = self.aligner._ops.handle.align_device(t, dets, counts, S)
        crops = crops.view(n * F, S, S, 3)
        if gate == "device":
            return self._recognize_gated(dets, counts, ok, crops, n, F, top_k)
        blur = self.quality._ops.handle.blur_scores_device(crops) if self.quality.check_blur else dets.new_empty(
            0, dtype=torch.float64)
        parts = [blur.view(torch.uint8), dets.view(-1).view(torch.uint8), counts.view(torch.uint8), ok.view(-1)]
        host = torch.cat(parts).cpu().numpy()  # the chain's one copy and its one synchronisation
        cut = np.cumsum([p.numel() for p in parts])
        h_blur = host[:cut[0]].view(np.float64).reshape(n, F) if self.quality.check_blur else None
        h_dets = host[cut[0]:cut[1]].view(np.float32).reshape(n, F, 15)
        h_counts = host[cut[1]:cut[2]].view(np.int32)
        h_ok = host[cut[2]:].reshape(n, F)
        for f in range(n):
            if h_counts[f] < 0:
                raise NotImplementedError(f"frame {f} has more than 4096 anchors above det_thresh (limit 4096)")
        out: List[List[Dict]] = []
        valid = []  # (frame, face) of the crops to embed, in output order
        for f in range(n):
            rows = []
            for i, d in enumerate(det._faces(h_dets[f], min(int(h_counts[f]), F))):
                good, q = self.quality.is_valid(d, None, None if h_blur is None else float(h_blur[f, i]))
                good = good and bool(h_ok[f, i])
                rows.append({"bbox": d.get("bbox"), "det_score": d["det_score"], "quality_metrics": q,
                             "is_valid": good, "matches": [], "recognized": False})
                if good:
                    valid.append((f, i))
            out.append(rows)
        if not valid:
            return out
        sel = crops[torch.tensor([f * F + i for f, i in valid], device=dev)].contiguous()
        res = self.gallery.match_resolved(len(valid), top_k, lambda h, k, idx, score: h.embed_match(sel, k, idx, score))
        for m, (f, i) in zip(res, valid):
            out[f][i]["matches"] = m
            out[f][i]["recognized"] = bool(m) and m[0][2] >= self.similarity_threshold
        return out


    def _recognize_gated(self, dets, counts, ok, crops, n: int, F: int, top_k: int) -> List[List[Dict]]:
        """``recognize_frames`` from the aligned slots on, with the gate on the device."""
        from .face_recognition import GATE_VALID, tensors_to_host
        blur = self.quality._ops.handle.blur_scores_device(crops) if self.quality.check_blur else None
        g = self.quality.gate_device(dets, counts, ok, blur)
        # the chain's one copy and its one synchronisation
        host = tensors_to_host({**{k: g[k] for k in ("stage", "metrics", "bbox", "valid_slots", "n_valid")},
                                "counts": counts})
        for f in range(n):
            if host["counts"][f] < 0:
                raise NotImplementedError(f"frame {f} has more than 4096 anchors above det_thresh (limit 4096)")
        out: List[List[Dict]] = []
        for f in range(n):
            rows = []
            for i in range(min(int(host["counts"][f]), F)):
                stage = host["stage"][f, i]
                q = self.quality.metrics_from_gate(stage, host["metrics"][f, i], host["bbox"][f, i])
                rows.append({"bbox": host["bbox"][f, i].copy(), "det_score": q["det_score"], "quality_metrics": q,
                             "is_valid": bool(stage == GATE_VALID), "matches": [], "recognized": False})
            out.append(rows)
        n_valid = int(host["n_valid"][0])
        if not n_valid:
            return out
        sel = crops[g["valid_slots"][:n_valid].long()].contiguous()
        res = self.gallery.match_resolved(n_valid, top_k, lambda h, k, idx, score: h.embed_match(sel, k, idx, score))
        for m, slot in zip(res, host["valid_slots"][:n_valid]):
            row = out[slot // F][slot % F]
            row["matches"] = m
            row["recognized"] = bool(m) and m[0][2] >= self.similarity_threshold
        return out


class MatchBatcher:
    """Dynamic batching of concurrent ``match_single_face`` calls.

    The reference server handles each request on its own Flask thread
    (``threaded=True``, ``face_recognition_server.py:1102``) and every one of them
    runs a batch-1 embed + search (``:321-323`` -> ``face_matcher.py:52-58``).  Here
    those threads call :meth:`match_single_face` (or :meth:`submit`) and one worker
    thread gathers whatever is pending -- up to ``max_batch`` crops, waiting at most
    ``max_wait_ms`` after the first -- into ONE ``FaceMatcher.match_faces`` call, i.e.
    one ``fr_embed_match`` (a replayed hipGraph when the batch is small).  Each
    caller gets what ``match_single_face`` would return, to fp32 summation order: the
    forward is batch-invariant within 1e-6 per embedding element (the stream-K schedule
    cuts a batch-size-dependent set of tiles along K), and the top-k kernel is exact
    with the same tie order, so the first ``top_k`` of a larger k are the top-``top_k``.

    Errors keep the reference behaviour per request: a crop of the wrong shape raises
    ``ValueError`` in the calling thread before it is queued; a failure of the batched
    call is raised in every caller of that batch.
    """

    def __init__(self, matcher, max_batch: int = 64, max_wait_ms: float = 2.0):
        if max_batch < 1:
            raise ValueError("max_batch must be >= 1")
        self.matcher = matcher
        self.max_batch = int(max_batch)
        self.max_wait = max(0.0, float(max_wait_ms)) / 1000.0
        self.batches: List[int] = []  # size of every batch run (for tests and monitoring)
        self._q: "queue.Queue[Optional[Tuple[np.ndarray, int, Future]]]" = queue.Queue()
        self._closed = False
        self._lock = threading.Lock()
        self._worker = threading.Thread(target=self._run, name="frhip-match-batcher", daemon=True)
        self._worker.start()

    def submit(self, face_image: np.ndarray, top_k: int = 5) -> Future:
        self.matcher.embedder._check_shape(face_image)
        fut: Future = Future()
        item = (np.ascontiguousarray(as_uint8_crop(face_image)), int(top_k), fut)
        with self._lock:
            if self._closed:
                raise RuntimeError("MatchBatcher is closed")
            self._q.put(item)
        return fut

    def match_single_face(self, face_image: np.ndarray, top_k: int = 5) -> List[Tuple[str, str, float]]:
        return self.submit(face_image, top_k).result()

    def close(self) -> None:
        """Finish every queued request, then stop the worker."""
        with self._lock:
            if self._closed:
                return
            self._closed = True
            self._q.put(None)
        self._worker.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _run(self) -> None:
        stop = False
        while not stop:
            item = self._q.get()
            if item is None:
                break
            batch = [item]
            deadline = time.monotonic() + self.max_wait
            while len(batch) < self.max_batch:
                try:
                    nxt = self._q.get(timeout=max(0.0, deadline - time.monotonic()))
                except queue.Empty:
                    break
                if nxt is None:
                    stop = True
                    break
                batch.append(nxt)
            self._serve(batch)

    def _serve(self, batch) -> None:
        self.batches.append(len(batch))
        try:
            n_rows = len(self.matcher.gallery.students)
            ks = [_slice_len(n_rows, k) for _, k, _ in batch]
            kmax = max(ks)
            if kmax == 0:
                res = [[] for _ in batch]
            else:
                res = self.matcher.match_faces([f for f, _, _ in batch], top_k=kmax)
        except BaseException as e:  # every caller of this batch sees the failure
            for _, _, fut in batch:
                fut.set_exception(e)
            return
        for (_, _, fut), r, k in zip(batch, res, ks):
            fut.set_result(r[:k])
