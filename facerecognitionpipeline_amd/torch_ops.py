"""PyTorch-ROCm operator surface of the hot path: ``torch.ops.frhip.*``.

SURVEY.md §8(b) asks for ``frhip::embed`` and ``frhip::match_topk`` as
``torch.library`` ops over PyTorch tensors, next to the C ABI.  They run the same
libfrhip entry points on the tensors' device and the current stream (no copy, no
CPU fallback).  A model or gallery is named by the integer id ``register``
returns for a ``FaceEmbedder`` / ``_lib.Handle``:

    hid = torch_ops.register(embedder)                       # once
    e = torch.ops.frhip.embed(rgb_u8_nhwc, hid, True)        # [N,512] f32
    idx, score = torch.ops.frhip.match_topk(e, hid, 5)       # [N,5] i32 / f32
    idx, score, e = torch.ops.frhip.embed_match(rgb, hid, 5)
    idx, score = torch.ops.frhip.match_identities(e, hid, "topk", 3, 5)   # identities of the sample gallery
    idx, score, e = torch.ops.frhip.embed_match_identities(rgb, hid, "topk", 3, 5)
    aug = torch.ops.frhip.augment_faces(crops_u8_nhwc, 8)    # [N,8,H,W,3] u8 (needs no model)
    rec_i, rec_d = torch.ops.frhip.track_consensus(idx, score, offsets, 0.55, 3, 0.5)  # [T,8] i32 / [T,2] f64
    face, fscore, image = torch.ops.frhip.photo_rollcall(idx, score, offsets, 0.35, 1)  # [N,4] i32, [N] f32, [P,4] i32
    tid, quality, slot, info = torch.ops.frhip.capture_tracks(bbox, metrics, valid, frame_offsets, clip_offsets,
                                                              30, 80.0, 12, 0.5, False)  # [N] x 3, [C,4] i32
    tid, prev, attempt, best, info = torch.ops.frhip.live_tracks(bbox, det_blur, frame_offsets, clip_offsets,
                                                                 100.0, 30, 3, 10)              # [N] x 4, [C,4] i32
    attempt, best, state, info = torch.ops.frhip.server_tracks(det_blur, clock, order, track_offsets,
                                                               3, 10, 10.0, 0.6)                # [N] x 3, [T,4] i32
    scores = torch.ops.frhip.identity_scores(q, gallery_rows, id_offsets, "mean", 3)   # [N, n_ids] f32
    rec_i, rec_f, counts = torch.ops.frhip.eval_probes(scores, true_id, thresholds)    # [N,4] x 2, [T,4] i64
    dets, counts = torch.ops.frhip.detect(frames_u8_nhwc, det_hid, 0.5, 16)            # [N,16,15] f32, [N] i32
    crops, tforms, ok = torch.ops.frhip.align_detections(frames, dets, counts, 112)    # [N,16,112,112,3] u8, f64, u8
    blur = torch.ops.frhip.blur_scores(crops.flatten(0, 1))                            # [N*16] f64
    dets, counts = torch.ops.frhip.detect_images([img0, img1], det_hid, 0.5, 16)       # images of different sizes
    crops, tforms, ok = torch.ops.frhip.align_image_detections([img0, img1], dets, counts, 112)

Each op has a fake (meta) implementation, so the ops trace under
``torch.fx`` / ``torch.export`` with the right output shapes.
"""
from __future__ import annotations

import itertools
import threading
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib

_handles: Dict[int, "_lib.Handle"] = {}
_ids = itertools.count(1)
_lock = threading.Lock()


def register(obj) -> int:
    """Id for a FaceEmbedder (its model handle) or a raw ``_lib.Handle``."""
    h = obj.model if hasattr(obj, "model") and isinstance(obj.model, _lib.Handle) else obj
    if not isinstance(h, _lib.Handle):
        raise TypeError("register() takes a FaceEmbedder or a facerecognitionpipeline_amd._lib.Handle")
    with _lock:
        hid = next(_ids)
        _handles[hid] = h
    return hid


def unregister(hid: int) -> None:
    with _lock:
        _handles.pop(hid, None)


def _get(hid: int) -> "_lib.Handle":
    try:
        return _handles[hid]
    except KeyError:
        raise ValueError(f"frhip handle id {hid} is not registered") from None


_utility: Dict[torch.device, "_lib.Handle"] = {}


def utility_handle(device) -> "_lib.Handle":
    """A model-less handle on ``device`` for the entry points that need no weights
    (``augment_faces``, ``track_consensus``, ``photo_rollcall``, ``capture_tracks``, ``live_tracks``, ``server_tracks``, ``identity_scores``, ``eval_probes``, ``align_detections``, ``align_image_detections``, ``blur_scores``): one per device, created on first use."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"facerecognitionpipeline_amd runs on a HIP device only (no CPU fallback); got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    with _lock:
        h = _utility.get(device)
        if h is None:
            h = _utility[device] = _lib.Handle("ir_50", "adaface", device, max_batch=1)
    return h


def _check_rgb(rgb: torch.Tensor, h: "_lib.Handle") -> torch.Tensor:
    if rgb.dtype != torch.uint8 or rgb.dim() != 4 or tuple(rgb.shape[1:]) != (112, 112, 3):
        raise ValueError("expected a uint8 [N,112,112,3] RGB tensor")
    if rgb.device != h.device:
        raise ValueError(f"input is on {rgb.device}, the model on {h.device} (no CPU fallback)")
    return rgb.contiguous()


@torch.library.custom_op("frhip::embed", mutates_args=())
def embed(rgb: torch.Tensor, handle: int, normalize: bool) -> torch.Tensor:
    h = _get(handle)
    rgb = _check_rgb(rgb, h)
    out = torch.empty((rgb.shape[0], 512), dtype=torch.float32, device=rgb.device)
    h.embed(rgb, out, normalize)
    return out


@embed.register_fake
def _(rgb, handle, normalize):
    return rgb.new_empty((rgb.shape[0], 512), dtype=torch.float32)


@torch.library.custom_op("frhip::match_topk", mutates_args=())
def match_topk(q: torch.Tensor, handle: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    h = _get(handle)
    if q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != 512 or q.device != h.device:
        raise ValueError("expected a float32 [N,512] query tensor on the model's device")
    q = q.contiguous()
    idx = torch.empty((q.shape[0], k), dtype=torch.int32, device=q.device)
    score = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    h.match(q, k, idx, score)
    return idx, score


@match_topk.register_fake
def _(q, handle, k):
    return (q.new_empty((q.shape[0], k), dtype=torch.int32), q.new_empty((q.shape[0], k), dtype=torch.float32))


@torch.library.custom_op("frhip::embed_match", mutates_args=())
def embed_match(rgb: torch.Tensor, handle: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    h = _get(handle)
    rgb = _check_rgb(rgb, h)
    n = rgb.shape[0]
    idx = torch.empty((n, k), dtype=torch.int32, device=rgb.device)
    score = torch.empty((n, k), dtype=torch.float32, device=rgb.device)
    emb = torch.empty((n, 512), dtype=torch.float32, device=rgb.device)
    h.embed_match(rgb, k, idx, score, emb)
    return idx, score, emb


@embed_match.register_fake
def _(rgb, handle, k):
    n = rgb.shape[0]
    return (rgb.new_empty((n, k), dtype=torch.int32), rgb.new_empty((n, k), dtype=torch.float32),
            rgb.new_empty((n, 512), dtype=torch.float32))


@torch.library.custom_op("frhip::match_identities", mutates_args=())
def match_identities(q: torch.Tensor, handle: int, aggregation: str, agg_k: int,
                     k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    h = _get(handle)
    if q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != 512 or q.device != h.device:
        raise ValueError("expected a float32 [N,512] query tensor on the handle's device")
    q = q.contiguous()
    idx = torch.empty((q.shape[0], k), dtype=torch.int32, device=q.device)
    score = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    h.match_identities(q, aggregation, agg_k, k, idx, score)
    return idx, score


@match_identities.register_fake
def _(q, handle, aggregation, agg_k, k):
    return (q.new_empty((q.shape[0], k), dtype=torch.int32), q.new_empty((q.shape[0], k), dtype=torch.float32))


@torch.library.custom_op("frhip::embed_match_identities", mutates_args=())
def embed_match_identities(rgb: torch.Tensor, handle: int, aggregation: str, agg_k: int,
                           k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    h = _get(handle)
    rgb = _check_rgb(rgb, h)
    n = rgb.shape[0]
    idx = torch.empty((n, k), dtype=torch.int32, device=rgb.device)
    score = torch.empty((n, k), dtype=torch.float32, device=rgb.device)
    emb = torch.empty((n, 512), dtype=torch.float32, device=rgb.device)
    h.embed_match_identities(rgb, aggregation, agg_k, k, idx, score, emb)
    return idx, score, emb


@embed_match_identities.register_fake
def _(rgb, handle, aggregation, agg_k, k):
    n = rgb.shape[0]
    return (rgb.new_empty((n, k), dtype=torch.int32), rgb.new_empty((n, k), dtype=torch.float32),
            rgb.new_empty((n, 512), dtype=torch.float32))


@torch.library.custom_op("frhip::augment_faces", mutates_args=())
def augment_faces(crops: torch.Tensor, num_augmentations: int) -> torch.Tensor:
    if crops.device.type != "cuda":
        raise ValueError(f"crops are on {crops.device}: augment_faces runs on a HIP device (no CPU fallback)")
    return utility_handle(crops.device).augment_faces(crops, num_augmentations)


@augment_faces.register_fake
def _(crops, num_augmentations):
    return crops.new_empty((crops.shape[0], num_augmentations, crops.shape[1], crops.shape[2], 3), dtype=torch.uint8)


@torch.library.custom_op("frhip::track_consensus", mutates_args=())
def track_consensus(idx: torch.Tensor, score: torch.Tensor, offsets: List[int], min_quality: float,
                    min_frames: int, similarity_threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    if idx.device.type != "cuda":
        raise ValueError(f"idx is on {idx.device}: track_consensus runs on a HIP device (no CPU fallback)")
    return utility_handle(idx.device).track_consensus(idx, score, offsets, min_quality, min_frames,
                                                      similarity_threshold)


@track_consensus.register_fake
def _(idx, score, offsets, min_quality, min_frames, similarity_threshold):
    t = max(len(offsets) - 1, 0)
    return idx.new_empty((t, 8), dtype=torch.int32), idx.new_empty((t, 2), dtype=torch.float64)


@torch.library.custom_op("frhip::photo_rollcall", mutates_args=())
def photo_rollcall(idx: torch.Tensor, score: torch.Tensor, offsets: List[int], similarity_threshold: float,
                   mode: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if idx.device.type != "cuda":
        raise ValueError(f"idx is on {idx.device}: photo_rollcall runs on a HIP device (no CPU fallback)")
    return utility_handle(idx.device).photo_rollcall(idx, score, offsets, similarity_threshold, mode)


@photo_rollcall.register_fake
def _(idx, score, offsets, similarity_threshold, mode):
    n, p = idx.shape[0], max(len(offsets) - 1, 0)
    return (idx.new_empty((n, 4), dtype=torch.int32), idx.new_empty((n,), dtype=torch.float32),
            idx.new_empty((p, 4), dtype=torch.int32))


@torch.library.custom_op("frhip::capture_tracks", mutates_args=())
def capture_tracks(bbox: torch.Tensor, metrics: torch.Tensor, valid: torch.Tensor, frame_offsets: List[int],
                   clip_offsets: List[int], max_disappeared: int, max_distance: float, target_frames: int,
                   min_quality_score: float, save_partial: bool
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    if bbox.device.type != "cuda":
        raise ValueError(f"bbox is on {bbox.device}: capture_tracks runs on a HIP device (no CPU fallback)")
    return utility_handle(bbox.device).capture_tracks(bbox, metrics, valid, frame_offsets, clip_offsets,
                                                      max_disappeared, max_distance, target_frames,
                                                      min_quality_score, save_partial)


@capture_tracks.register_fake
def _(bbox, metrics, valid, frame_offsets, clip_offsets, max_disappeared, max_distance, target_frames,
      min_quality_score, save_partial):
    n, c = bbox.shape[0], max(len(clip_offsets) - 1, 0)
    return (bbox.new_empty((n,), dtype=torch.int32), bbox.new_empty((n,), dtype=torch.float64),
            bbox.new_empty((n,), dtype=torch.int32), bbox.new_empty((c, 4), dtype=torch.int32))


@torch.library.custom_op("frhip::live_tracks", mutates_args=())
def live_tracks(bbox: torch.Tensor, metrics: torch.Tensor, frame_offsets: List[int], clip_offsets: List[int],
                max_distance: float, recognition_interval: int, max_attempts: int, buffer_size: int
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    if bbox.device.type != "cuda":
        raise ValueError(f"bbox is on {bbox.device}: live_tracks runs on a HIP device (no CPU fallback)")
    return utility_handle(bbox.device).live_tracks(bbox, metrics, frame_offsets, clip_offsets, max_distance,
                                                   recognition_interval, max_attempts, buffer_size)


@live_tracks.register_fake
def _(bbox, metrics, frame_offsets, clip_offsets, max_distance, recognition_interval, max_attempts, buffer_size):
    n, c = bbox.shape[0], max(len(clip_offsets) - 1, 0)
    return (bbox.new_empty((n,), dtype=torch.int32), bbox.new_empty((n,), dtype=torch.int32),
            bbox.new_empty((n,), dtype=torch.int32), bbox.new_empty((n,), dtype=torch.int32),
            bbox.new_empty((c, 4), dtype=torch.int32))


@torch.library.custom_op("frhip::server_tracks", mutates_args=())
def server_tracks(metrics: torch.Tensor, clock: torch.Tensor, order: torch.Tensor, track_offsets: List[int],
                  max_attempts: int, buffer_size: int, retry_cooldown: float, det_gate: float
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    if metrics.device.type != "cuda":
        raise ValueError(f"metrics are on {metrics.device}: server_tracks runs on a HIP device (no CPU fallback)")
    return utility_handle(metrics.device).server_tracks(metrics, clock, order, track_offsets, max_attempts,
                                                        buffer_size, retry_cooldown, det_gate)


@server_tracks.register_fake
def _(metrics, clock, order, track_offsets, max_attempts, buffer_size, retry_cooldown, det_gate):
    n, t = metrics.shape[0], max(len(track_offsets) - 1, 0)
    return (metrics.new_empty((n,), dtype=torch.int32), metrics.new_empty((n,), dtype=torch.int32),
            metrics.new_empty((n,), dtype=torch.int32), metrics.new_empty((t, 4), dtype=torch.int32))


@torch.library.custom_op("frhip::identity_scores", mutates_args=())
def identity_scores(q: torch.Tensor, gallery: torch.Tensor, offsets: List[int], aggregation: str,
                    k: int) -> torch.Tensor:
    if q.device.type != "cuda":
        raise ValueError(f"q is on {q.device}: identity_scores runs on a HIP device (no CPU fallback)")
    return utility_handle(q.device).identity_scores(q, gallery, offsets, aggregation, k)


@identity_scores.register_fake
def _(q, gallery, offsets, aggregation, k):
    return q.new_empty((q.shape[0], max(len(offsets) - 1, 0)), dtype=torch.float32)


@torch.library.custom_op("frhip::eval_probes", mutates_args=())
def eval_probes(scores: torch.Tensor, true_id: torch.Tensor,
                thresholds: List[float]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if scores.device.type != "cuda":
        raise ValueError(f"scores are on {scores.device}: eval_probes runs on a HIP device (no CPU fallback)")
    return utility_handle(scores.device).eval_probes(scores, true_id, thresholds)


@eval_probes.register_fake
def _(scores, true_id, thresholds):
    n = scores.shape[0]
    return (scores.new_empty((n, 4), dtype=torch.int32), scores.new_empty((n, 4), dtype=torch.float32),
            scores.new_empty((len(thresholds), 4), dtype=torch.int64))


# The frames -> (detections, crops, blur) chain on device tensors: no host copy and no
# synchronisation in any of the three (fr_detect_device / fr_align_device / fr_blur_scores_device).
@torch.library.custom_op("frhip::detect", mutates_args=())
def detect(frames: torch.Tensor, handle: int, det_thresh: float, max_faces: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return _get(handle).detect_device(frames, det_thresh, max_faces)


@detect.register_fake
def _(frames, handle, det_thresh, max_faces):
    n = frames.shape[0]
    return frames.new_empty((n, max_faces, 15), dtype=torch.float32), frames.new_empty((n,), dtype=torch.int32)


@torch.library.custom_op("frhip::align_detections", mutates_args=())
def align_detections(frames: torch.Tensor, dets: torch.Tensor, counts: torch.Tensor,
                     out_size: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if frames.device.type != "cuda":
        raise ValueError(f"frames are on {frames.device}: align_detections runs on a HIP device (no CPU fallback)")
    if dets.dim() != 3 or dets.shape[2] != 15:
        raise ValueError("expected detection rows float32 [N,F,15] (frhip::detect's dets)")
    return utility_handle(frames.device).align_device(frames, dets, counts, out_size)


@align_detections.register_fake
def _(frames, dets, counts, out_size):
    n, f = dets.shape[0], dets.shape[1]
    return (frames.new_empty((n, f, out_size, out_size, 3), dtype=torch.uint8),
            frames.new_empty((n, f, 2, 3), dtype=torch.float64), frames.new_empty((n, f), dtype=torch.uint8))


# The same two for images of different sizes (fr_detect_images_device / fr_align_images_device):
# a list of uint8 [H,W,3] tensors, outputs as ``detect`` / ``align_detections`` give them.
@torch.library.custom_op("frhip::detect_images", mutates_args=())
def detect_images(images: List[torch.Tensor], handle: int, det_thresh: float,
                  max_faces: int) -> Tuple[torch.Tensor, torch.Tensor]:
    for i, im in enumerate(images):
        if im.device.type != "cuda":
            raise ValueError(f"image {i} is on {im.device}: detect_images runs on a HIP device (no CPU fallback)")
    return _get(handle).detect_images_device(images, det_thresh, max_faces)


@detect_images.register_fake
def _(images, handle, det_thresh, max_faces):
    n = len(images)
    dev = images[0].device if n else _get(handle).device
    return (torch.empty((n, max_faces, 15), dtype=torch.float32, device=dev),
            torch.empty((n,), dtype=torch.int32, device=dev))


@torch.library.custom_op("frhip::align_image_detections", mutates_args=())
def align_image_detections(images: List[torch.Tensor], dets: torch.Tensor, counts: torch.Tensor,
                           out_size: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    for i, im in enumerate(images):
        if im.device.type != "cuda":
            raise ValueError(f"image {i} is on {im.device}: align_image_detections runs on a HIP device "
                             "(no CPU fallback)")
    if dets.device.type != "cuda":
        raise ValueError(f"dets are on {dets.device}: align_image_detections runs on a HIP device (no CPU fallback)")
    if dets.dim() != 3 or dets.shape[2] != 15:
        raise ValueError("expected detection rows float32 [N,F,15] (frhip::detect_images' dets)")
    return utility_handle(dets.device).align_images_device(images, dets, counts, out_size)


@align_image_detections.register_fake
def _(images, dets, counts, out_size):
    n, f = dets.shape[0], dets.shape[1]
    return (dets.new_empty((n, f, out_size, out_size, 3), dtype=torch.uint8),
            dets.new_empty((n, f, 2, 3), dtype=torch.float64), dets.new_empty((n, f), dtype=torch.uint8))


@torch.library.custom_op("frhip::blur_scores", mutates_args=())
def blur_scores(crops: torch.Tensor) -> torch.Tensor:
    if crops.device.type != "cuda":
        raise ValueError(f"crops are on {crops.device}: blur_scores runs on a HIP device (no CPU fallback)")
    return utility_handle(crops.device).blur_scores_device(crops)


@blur_scores.register_fake
def _(crops):
    return crops.new_empty((crops.shape[0],), dtype=torch.float64)


# The quality gate behind them (fr_quality_gate_device): ``limits`` = min_det_score, min_face_size,
# max_yaw, max_pitch, max_roll, blur_threshold; the outputs in _lib.GATE_OUTPUTS order.
_GateOut = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                 torch.Tensor]


@torch.library.custom_op("frhip::quality_gate", mutates_args=())
def quality_gate(dets: torch.Tensor, counts: Optional[torch.Tensor], ok: Optional[torch.Tensor],
                 blur: Optional[torch.Tensor], limits: List[float], check_blur: bool) -> _GateOut:
    if dets.device.type != "cuda":
        raise ValueError(f"dets are on {dets.device}: quality_gate runs on a HIP device (no CPU fallback)")
    if len(limits) != 6:
        raise ValueError("limits: min_det_score, min_face_size, max_yaw, max_pitch, max_roll, blur_threshold")
    config = dict(zip(("min_det_score", "min_face_size", "max_yaw", "max_pitch", "max_roll", "blur_threshold"),
                      limits), check_blur=check_blur)
    out = utility_handle(dets.device).quality_gate_device(dets, counts, ok, blur, config)
    return tuple(out[k] for k in _lib.GATE_OUTPUTS)


@quality_gate.register_fake
def _(dets, counts, ok, blur, limits, check_blur):
    n, f = dets.shape[0], dets.shape[1]
    new = dets.new_empty
    return (new((n, f), dtype=torch.uint8), new((n, f, 5), dtype=torch.float64), new((n, f, 4), dtype=torch.int32),
            new((n, f), dtype=torch.int32), new((n * f,), dtype=torch.int32), new((n + 1,), dtype=torch.int32),
            new((n * f,), dtype=torch.int32), new((1,), dtype=torch.int32))
