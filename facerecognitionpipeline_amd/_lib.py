"""ctypes binding of libfrhip.so (the C ABI of include/frhip.h).

The library is loaded AFTER ``import torch`` so that it binds to the same HIP
runtime instance (SONAME libamdhip64.so.7) PyTorch-ROCm already loaded: device
pointers and streams are then shared with torch tensors.  There is no CPU
fallback anywhere: if the library is missing or no GPU is present, every
entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional

import torch  # noqa: F401  (must precede the CDLL load, see module doc)

# FRHIP_LIB: another build of the library (tools' A/B of two builds in one tree); default: in-tree
LIB_PATH = os.environ.get("FRHIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfrhip.so")

FR_OK = 0
FR_ERR_INVALID_ARGUMENT = -1
FR_ERR_MISSING_PARAM = -2
FR_ERR_HIP = -3
FR_ERR_STATE = -4
FR_ERR_UNSUPPORTED = -5

_P = ctypes.c_void_p
_I = ctypes.c_int
_SIGNATURES = {
    "fr_create": (_I, [ctypes.c_char_p, ctypes.c_char_p, _I, _I, ctypes.POINTER(_P)]),
    "fr_destroy": (_I, [_P]),
    "fr_set_param": (_I, [_P, ctypes.c_char_p, _P, ctypes.c_int64]),
    "fr_finalize": (_I, [_P]),
    "fr_embed": (_I, [_P, _P, _I, _I, _I, _P, _I, _P]),
    "fr_embed_host": (_I, [_P, _P, _I, _I, _I, _P, _I]),
    "fr_resize_crops": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "fr_resize_images": (_I, [_P, _P, _P, _I, _P, _P]),
    "fr_embed_images": (_I, [_P, _P, _P, _I, _P, _I, _P]),
    "fr_augment_faces": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "fr_gallery_set": (_I, [_P, _P, _I, _I, _I, _P]),
    "fr_gallery_size": (_I, [_P, ctypes.POINTER(_I)]),
    "fr_gallery_write_rows": (_I, [_P, _I, _I, _P, _I, _P]),
    "fr_gallery_delete_rows": (_I, [_P, _I, _I, _P]),
    "fr_gallery_read": (_I, [_P, _I, _I, _P, _I, _P]),
    "fr_build_templates": (_I, [_P, _P, _P, _I, _I, ctypes.c_float, _P, _P, _P]),
    "fr_track_consensus": (_I, [_P, _P, _P, _I, _P, _I, ctypes.c_double, _I, ctypes.c_double, _P, _P, _P]),
    "fr_photo_rollcall": (_I, [_P, _P, _P, _I, _P, _I, ctypes.c_double, _I, _P, _P, _P, _P]),
    "fr_capture_tracks": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, ctypes.c_double, _I, ctypes.c_double, _I, _P, _P, _P,
                               _P, _P]),
    "fr_live_tracks": (_I, [_P, _P, _P, _P, _P, _I, ctypes.c_double, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "fr_server_tracks": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double, _P, _P, _P, _P,
                              _P]),
    "fr_identity_scores": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P]),
    "fr_eval_probes": (_I, [_P, _P, _I, _I, _P, _P, _I, _P, _P, _P, _P]),
    "fr_samples_set": (_I, [_P, _P, _P, _I, _I, _P]),
    "fr_samples_size": (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "fr_match_identities": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "fr_embed_match_identities": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "fr_match_topk": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "fr_match_topk_host": (_I, [_P, _P, _I, _I, _P, _P]),
    "fr_embed_match": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "fr_align_faces": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P]),
    "fr_warp_affine": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _P]),
    "fr_blur_scores": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "fr_detect": (_I, [_P, _P, _I, _I, _I, ctypes.c_float, _I, _P, _P, _P]),
    "fr_detect_images": (_I, [_P, _P, _P, _I, ctypes.c_float, _I, _P, _P, _P]),
    "fr_align_images": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P]),
    "fr_detect_device": (_I, [_P, _P, _I, _I, _I, ctypes.c_float, _I, _P, _P, _P]),
    "fr_align_device": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P]),
    "fr_detect_images_device": (_I, [_P, _P, _P, _I, ctypes.c_float, _I, _P, _P, _P]),
    "fr_align_images_device": (_I, [_P, _P, _P, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P]),
    "fr_blur_scores_device": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "fr_quality_gate_device": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fr_set_precision": (_I, [_P, _I]),
    "fr_set_conv_algorithm": (_I, [_P, _I]),
    "fr_set_graph_batch": (_I, [_P, _I]),
    "fr_set_lanes": (_I, [_P, _I, _I]),
    "fr_graph_count": (_I, [_P, ctypes.POINTER(ctypes.c_int)]),
    "fr_get_lanes": (_I, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "fr_profile_enable": (_I, [_P, _I]),
    "fr_profile_kernel": (_I, [_P, _I, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "fr_profile_read": (_I, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]),
    "fr_last_error": (ctypes.c_char_p, [_P]),
    "fr_version": (ctypes.c_char_p, []),
}



class GateConfig(ctypes.Structure):
    """fr_gate_config."""
    _fields_ = [(k, ctypes.c_double) for k in ("min_det_score", "min_face_size", "max_yaw", "max_pitch", "max_roll",
                                               "blur_threshold")] + [("check_blur", ctypes.c_int)]


GATE_OUTPUTS = ("stage", "metrics", "bbox", "rank", "rows", "frame_offsets", "valid_slots", "n_valid")

_lib: Optional[ctypes.CDLL] = None
_lock = threading.Lock()


class FrHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libfrhip.so once; raise loudly if it is not built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise FrHipError(f"{LIB_PATH} is not built: run `python -m facerecognitionpipeline_amd.build` "
                                 "(the HIP path has no CPU fallback)")
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in _SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(rc: int, handle=None) -> None:
    """Map a status code to the reference's exception types (SURVEY.md §8(b) Errors)."""
    if rc == FR_OK:
        return
    msg = load().fr_last_error(handle)
    msg = msg.decode() if msg else f"frhip error {rc}"
    if rc == FR_ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    if rc == FR_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise FrHipError(msg)


def ptr(t) -> Optional[int]:
    """Raw data pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_of(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _csr_offsets(offsets, end=None, message="", min_slices=0):
    """CSR offsets as a contiguous int32 vector and its slice count; ``ValueError(message)`` for fewer
    than ``min_slices`` slices or, with ``end``, slices that do not end at it."""
    import numpy as np
    off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
    n = off.shape[0] - 1
    if end is not None and (n < min_slices or (n > 0 and int(off[-1]) != end)):
        raise ValueError(message)
    return off, n


class Handle:
    """Owns one ``fr_handle``: a model (after ``load_state_dict``) and/or a gallery."""

    def __init__(self, architecture: str, model_type: str, device: torch.device, max_batch: int = 256):
        if device.type != "cuda":
            raise RuntimeError("facerecognitionpipeline_amd runs on a HIP device only (no CPU fallback); "
                               f"got device={device}")
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: the MI355X hot path has no CPU fallback")
        self.device = device
        self._lib = load()
        h = _P()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.max_batch = int(max_batch)  # for a detector: max_frames, the images of one chunk
        self.gallery_tag = None  # (owner, version) of the rows in HBM; see GalleryManager._sync_device
        self.samples_tag = None  # the same for the sample gallery; see GalleryManager._sync_samples
        check(self._lib.fr_create(architecture.encode(), model_type.encode(), idx, int(max_batch), ctypes.byref(h)))
        self.h = h

    def _require_device(self, name: str, *tensors) -> None:
        """``name`` names the tensors, e.g. "idx / score"."""
        if any(x.device != self.device for x in tensors):
            raise ValueError(f"{name} {'is' if len(tensors) == 1 else 'are'} on "
                             f"{' / '.join(str(x.device) for x in tensors)}, the handle on {self.device} "
                             "(no CPU fallback)")

    def close(self) -> None:
        if getattr(self, "h", None) and self._lib is not None:
            self._lib.fr_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    # -- model -------------------------------------------------------------
    def load_state_dict(self, state_dict) -> None:
        import numpy as np
        for k, v in state_dict.items():
            a = np.ascontiguousarray(np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v),
                                     dtype=np.float32)
            check(self._lib.fr_set_param(self.h, k.encode(), a.ctypes.data, a.size), self.h)
        check(self._lib.fr_finalize(self.h), self.h)

    def embed(self, rgb: torch.Tensor, out: torch.Tensor, normalize: bool = True) -> None:
        n = rgb.shape[0]
        check(self._lib.fr_embed(self.h, ptr(rgb), n, rgb.shape[1], rgb.shape[2], ptr(out), int(normalize),
                                 stream_of(self.device)), self.h)

    def resize_crops(self, src: torch.Tensor, out: torch.Tensor) -> None:
        """cv2.resize(INTER_LINEAR) of uint8 [n,H,W,3] device crops into out [n,112,112,3]."""
        check(self._lib.fr_resize_crops(self.h, ptr(src), src.shape[0], src.shape[1], src.shape[2], ptr(out),
                                        stream_of(self.device)), self.h)

    def augment_faces(self, crops: torch.Tensor, num_augmentations: int = 8,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The first ``num_augmentations`` (1..14) entries of the reference's
        ``augment_face_for_enrollment`` list for every uint8 [n,H,W,3] device crop -> uint8
        [n,A,H,W,3]; ``reshape(n * A, H, W, 3)`` is the reference's ``all_face_images`` order."""
        if crops.dtype != torch.uint8 or crops.dim() != 4 or crops.shape[3] != 3:
            raise ValueError("expected uint8 [n,H,W,3] RGB crops")
        if crops.device != self.device:
            raise ValueError(f"crops are on {crops.device}, the handle on {self.device} (no CPU fallback)")
        crops = crops.contiguous()
        n, H, W = crops.shape[0], crops.shape[1], crops.shape[2]
        A = int(num_augmentations)
        shape = (n, max(A, 0), H, W, 3)
        if out is None:
            out = torch.empty(shape if 1 <= A <= 14 else (0,), dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 {list(shape)} tensor on {self.device}")
        check(self._lib.fr_augment_faces(self.h, ptr(crops), n, H, W, A, ptr(out), stream_of(self.device)), self.h)
        return out

    # -- gallery -----------------------------------------------------------
    def gallery_set(self, E: torch.Tensor, tag=None) -> None:
        G = E.shape[0] if E.numel() else 0
        D = E.shape[1] if E.dim() == 2 else 512
        check(self._lib.fr_gallery_set(self.h, ptr(E) if G else None, G, D, 1, stream_of(self.device)), self.h)
        self.gallery_tag = tag

    def gallery_replace(self, E: torch.Tensor) -> None:
        """Replace the rows with a device [G,512] matrix built from the current ones (a delta
        replay's compaction; the gallery tag is left to the caller)."""
        E = E.contiguous()
        G = E.shape[0]
        check(self._lib.fr_gallery_set(self.h, ptr(E) if G else None, G, 512, 1, stream_of(self.device)), self.h)

    def gallery_size(self) -> int:
        g = ctypes.c_int()
        check(self._lib.fr_gallery_size(self.h, ctypes.byref(g)), self.h)
        return g.value

    def gallery_write_rows(self, row0: int, E: torch.Tensor) -> None:
        """Rows [row0, row0 + len(E)) := E (device f32 [n,512]); may extend the gallery."""
        E = E.to(device=self.device, dtype=torch.float32).contiguous()
        check(self._lib.fr_gallery_write_rows(self.h, int(row0), E.shape[0], ptr(E), 1, stream_of(self.device)),
              self.h)

    def gallery_delete_rows(self, row0: int, n: int = 1) -> None:
        check(self._lib.fr_gallery_delete_rows(self.h, int(row0), int(n), stream_of(self.device)), self.h)

    def gallery_read(self) -> torch.Tensor:
        G = self.gallery_size()
        out = torch.empty((G, 512), dtype=torch.float32, device=self.device)
        check(self._lib.fr_gallery_read(self.h, 0, G, ptr(out) if G else None, 1, stream_of(self.device)), self.h)
        return out

    def build_templates(self, emb: torch.Tensor, offsets, method: str = "mean", min_similarity: float = 0.70):
        """Templates of len(offsets)-1 students whose samples are CSR rows of ``emb`` [total,512]
        -> (templates f32 [S,512], kept int32 [S]) on the device."""
        methods = {"mean": 0, "median": 1, "weighted_mean": 2}
        m = methods.get(method, 0)  # the reference falls back to mean for unknown methods
        off, S = _csr_offsets(offsets)
        emb = emb.to(device=self.device, dtype=torch.float32).contiguous()
        tpl = torch.empty((max(S, 0), 512), dtype=torch.float32, device=self.device)
        kept = torch.empty((max(S, 0),), dtype=torch.int32, device=self.device)
        check(self._lib.fr_build_templates(self.h, ptr(emb), off.ctypes.data, S, m, float(min_similarity), ptr(tpl),
                                           ptr(kept), stream_of(self.device)), self.h)
        return tpl, kept

    def match(self, Q: torch.Tensor, k: int, idx: torch.Tensor, score: torch.Tensor) -> None:
        check(self._lib.fr_match_topk(self.h, ptr(Q), Q.shape[0], int(k), ptr(idx), ptr(score),
                                      stream_of(self.device)), self.h)

    def embed_match(self, rgb: torch.Tensor, k: int, idx: torch.Tensor, score: torch.Tensor,
                    emb: Optional[torch.Tensor] = None) -> None:
        check(self._lib.fr_embed_match(self.h, ptr(rgb), rgb.shape[0], int(k), ptr(idx), ptr(score), ptr(emb),
                                       stream_of(self.device)), self.h)

    def track_consensus(self, idx: torch.Tensor, score: torch.Tensor, offsets, min_quality: float = 0.55,
                        min_frames: int = 3, similarity_threshold: float = 0.5):
        """The reference's track vote (``FaceMatcher._aggregate_matches`` / ``_get_best_candidate``)
        for len(offsets)-1 tracks whose frames are CSR rows of the device top-k output ``idx`` int32 /
        ``score`` float32 [total,k] -> (int32 [T,8] = status, winner row, winner count, pool size,
        second count, frames, quality frames, 0; float64 [T,2] = confidence, ratio) on the device."""
        if (idx.dim() != 2 or idx.dtype != torch.int32 or score.dtype != torch.float32
                or tuple(score.shape) != tuple(idx.shape)):
            raise ValueError("expected idx int32 [total,k] and score float32 [total,k]")
        self._require_device("idx / score", idx, score)
        off, T = _csr_offsets(offsets, idx.shape[0], f"offsets must end at the {idx.shape[0]} rows of idx / score")
        idx, score = idx.contiguous(), score.contiguous()
        out_i = torch.empty((T, 8), dtype=torch.int32, device=self.device)
        out_d = torch.empty((T, 2), dtype=torch.float64, device=self.device)
        check(self._lib.fr_track_consensus(self.h, ptr(idx), ptr(score), idx.shape[1], off.ctypes.data, T,
                                           float(min_quality), int(min_frames), float(similarity_threshold),
                                           ptr(out_i), ptr(out_d), stream_of(self.device)), self.h)
        return out_i, out_d

    def photo_rollcall(self, idx: torch.Tensor, score: torch.Tensor, offsets, similarity_threshold: float = 0.5,
                       mode: int = 0):
        """Who is in each photograph (include/frhip.h, fr_photo_rollcall): len(offsets)-1 photographs
        whose faces are CSR rows (0..1024 each) of the device top-k output ``idx`` int32 / ``score``
        float32 [total,k]; ``mode`` 0 (FR_ROLLCALL_INDEPENDENT: the reference's top-1 rule per face) or
        1 (FR_ROLLCALL_EXCLUSIVE: a row goes to at most one face of a photograph) -> (out_face int32
        [total,4] = status, row, column, 0; out_score float32 [total]; out_image int32 [P,4] = faces,
        recognized, candidates, displaced) on the device."""
        if (idx.dim() != 2 or idx.dtype != torch.int32 or score.dtype != torch.float32
                or tuple(score.shape) != tuple(idx.shape)):
            raise ValueError("expected idx int32 [total,k] and score float32 [total,k]")
        self._require_device("idx / score", idx, score)
        off, P = _csr_offsets(offsets)
        if P < 0 or int(off[-1]) != idx.shape[0]:  # also without photographs
            raise ValueError(f"offsets must end at the {idx.shape[0]} rows of idx / score")
        idx, score = idx.contiguous(), score.contiguous()
        total = idx.shape[0]
        out_face = torch.empty((total, 4), dtype=torch.int32, device=self.device)
        out_score = torch.empty((total,), dtype=torch.float32, device=self.device)
        out_image = torch.empty((P, 4), dtype=torch.int32, device=self.device)
        check(self._lib.fr_photo_rollcall(self.h, ptr(idx) if total else None, ptr(score) if total else None,
                                          idx.shape[1], off.ctypes.data, P, float(similarity_threshold), int(mode),
                                          ptr(out_face) if total else None, ptr(out_score) if total else None,
                                          ptr(out_image), stream_of(self.device)), self.h)
        return out_face, out_score, out_image

    def capture_tracks(self, bbox: torch.Tensor, metrics: torch.Tensor, valid: torch.Tensor, frame_offsets,
                       clip_offsets=None, max_disappeared: int = 30, max_distance: float = 50,
                       target_frames: int = 12, min_quality_score: float = 0.5, save_partial: bool = False,
                       raise_on_clip_error: bool = True):
        """The reference's ``SimpleTracker.update`` + ``FrameAccumulator`` (face_detection.py:11-228)
        for len(clip_offsets)-1 capture sessions in one launch.  ``bbox`` int32 [total,4], ``metrics``
        float64 [total,5] (det_score, blur_score, yaw, pitch, roll) and ``valid`` uint8 / bool [total]
        on the device; frame f = detections [frame_offsets[f], frame_offsets[f+1]), clip c = frames
        [clip_offsets[c], clip_offsets[c+1]) (default: one clip of all frames) -> (track_id int32
        [total], quality float64 [total], slot int32 [total], clip_info int32 [C,4] = tracks opened,
        tracks completed, frames saved, error) on the device.  A clip past the kernel's limits raises
        NotImplementedError; with ``raise_on_clip_error=False`` the outputs are returned instead and
        ``clip_info[:, 3]`` names the clips (their track_id is 0 and slot -1 throughout)."""
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        if (bbox.dim() != 2 or bbox.shape[1] != 4 or bbox.dtype != torch.int32 or metrics.dtype != torch.float64
                or tuple(metrics.shape) != (bbox.shape[0], 5) or valid.dtype != torch.uint8
                or tuple(valid.shape) != (bbox.shape[0],)):
            raise ValueError("expected bbox int32 [total,4], metrics float64 [total,5] and valid uint8 [total]")
        for name, x in (("bbox", bbox), ("metrics", metrics), ("valid", valid)):
            self._require_device(name, x)
        fo, F = _csr_offsets(frame_offsets)
        if F < 0:
            raise ValueError("frame_offsets needs at least its leading 0")
        co, C = _csr_offsets([0, F] if clip_offsets is None else clip_offsets, F,
                             f"clip_offsets must end at the {F} frames of frame_offsets")
        if int(fo[-1]) != bbox.shape[0]:  # also without frames
            raise ValueError(f"frame_offsets must end at the {bbox.shape[0]} rows of bbox / metrics / valid")
        bbox, metrics, valid = bbox.contiguous(), metrics.contiguous(), valid.contiguous()
        total = bbox.shape[0]
        track_id = torch.empty((total,), dtype=torch.int32, device=self.device)
        quality = torch.empty((total,), dtype=torch.float64, device=self.device)
        slot = torch.empty((total,), dtype=torch.int32, device=self.device)
        info = torch.empty((max(C, 0), 4), dtype=torch.int32, device=self.device)
        rc = self._lib.fr_capture_tracks(self.h, ptr(bbox), ptr(metrics), ptr(valid), fo.ctypes.data, co.ctypes.data,
                                         C, int(max_disappeared), float(max_distance), int(target_frames),
                                         float(min_quality_score), int(bool(save_partial)), ptr(track_id),
                                         ptr(quality), ptr(slot), ptr(info), stream_of(self.device))
        if rc != FR_ERR_UNSUPPORTED or raise_on_clip_error:
            check(rc, self.h)
        return track_id, quality, slot, info

    def live_tracks(self, bbox: torch.Tensor, metrics: torch.Tensor, frame_offsets, clip_offsets=None,
                    max_distance: float = 100, recognition_interval: int = 30, max_attempts: int = 3,
                    buffer_size: int = 10, raise_on_clip_error: bool = True):
        """The reference's ``LiveFaceRecognition._simple_track_assignment`` and the gating and frame
        selection of ``LiveRecognitionTracker`` (face_recognition_live.py:18-80, :249-285) for
        len(clip_offsets)-1 live sessions in one launch.  ``bbox`` int32 [total,4] and ``metrics``
        float64 [total,2] (det_score, blur_score) on the device; frames and clips as
        :meth:`capture_tracks` takes them -> (track_id int32 [total] from 0, prev int32 [total],
        attempt int32 [total], best int32 [total], clip_info int32 [C,4] = tracks opened, candidates,
        frames, error) on the device; ``prev`` and ``best`` are global detection indices, -1 for none.
        A clip past the coordinate limit raises NotImplementedError; with
        ``raise_on_clip_error=False`` the outputs are returned instead and ``clip_info[:, 3]`` names
        the clips (their track_id is 0 and the rest -1 throughout)."""
        if (bbox.dim() != 2 or bbox.shape[1] != 4 or bbox.dtype != torch.int32 or metrics.dtype != torch.float64
                or tuple(metrics.shape) != (bbox.shape[0], 2)):
            raise ValueError("expected bbox int32 [total,4] and metrics float64 [total,2]")
        for name, x in (("bbox", bbox), ("metrics", metrics)):
            self._require_device(name, x)
        fo, F = _csr_offsets(frame_offsets)
        if F < 0:
            raise ValueError("frame_offsets needs at least its leading 0")
        co, C = _csr_offsets([0, F] if clip_offsets is None else clip_offsets, F,
                             f"clip_offsets must end at the {F} frames of frame_offsets")
        if int(fo[-1]) != bbox.shape[0]:  # also without frames
            raise ValueError(f"frame_offsets must end at the {bbox.shape[0]} rows of bbox / metrics")
        bbox, metrics = bbox.contiguous(), metrics.contiguous()
        total = bbox.shape[0]
        track_id, prev, attempt, best = (torch.empty((total,), dtype=torch.int32, device=self.device)
                                         for _ in range(4))
        info = torch.empty((max(C, 0), 4), dtype=torch.int32, device=self.device)
        rc = self._lib.fr_live_tracks(self.h, ptr(bbox), ptr(metrics), fo.ctypes.data, co.ctypes.data, C,
                                      float(max_distance), int(recognition_interval), int(max_attempts),
                                      int(buffer_size), ptr(track_id), ptr(prev), ptr(attempt), ptr(best), ptr(info),
                                      stream_of(self.device))
        if rc != FR_ERR_UNSUPPORTED or raise_on_clip_error:
            check(rc, self.h)
        return track_id, prev, attempt, best, info

    def server_tracks(self, metrics: torch.Tensor, clock: torch.Tensor, order: torch.Tensor, track_offsets,
                      max_attempts: int = 3, buffer_size: int = 10, retry_cooldown: float = 10.0,
                      det_gate: float = 0.6, raise_on_track_error: bool = True):
        """The gating, the retry cooldown and the frame selection of the server's
        ``LiveRecognitionTracker`` (face_recognition_server.py:23-124) for every track of a recorded
        request log in one launch.  ``metrics`` float64 [n,2] (det_score, blur_score), ``clock``
        float64 [n] (the request's clock, repeated for its faces) and ``order`` int32 [n] (detection
        indices grouped by track, arrival order within a track) on the device; track t =
        ``order[track_offsets[t]:track_offsets[t+1]]`` -> (attempt int32 [n], best int32 [n], state
        int32 [n] of ``FR_SERVER_*``, track_info int32 [T,4] = attempts, cooldowns set, resets, error)
        on the device.  A track with a non-finite value or a bad ``order`` entry raises
        NotImplementedError; with ``raise_on_track_error=False`` the outputs are returned instead and
        ``track_info[:, 3]`` names the tracks (-1 / -1 / ``FR_SERVER_GATED`` throughout)."""
        if (metrics.dim() != 2 or metrics.shape[1] != 2 or metrics.dtype != torch.float64
                or clock.dtype != torch.float64 or tuple(clock.shape) != (metrics.shape[0],)
                or order.dtype != torch.int32 or order.dim() != 1):
            raise ValueError("expected metrics float64 [n,2], clock float64 [n] and order int32 [total]")
        for name, x in (("metrics", metrics), ("clock", clock), ("order", order)):
            self._require_device(name, x)
        off, T = _csr_offsets(track_offsets)
        if T < 0 or int(off[-1]) != order.shape[0]:
            raise ValueError(f"track_offsets must end at the {order.shape[0]} entries of order")
        metrics, clock, order = metrics.contiguous(), clock.contiguous(), order.contiguous()
        n = metrics.shape[0]
        attempt, best = (torch.full((n,), -1, dtype=torch.int32, device=self.device) for _ in range(2))
        state = torch.zeros((n,), dtype=torch.int32, device=self.device)
        info = torch.empty((T, 4), dtype=torch.int32, device=self.device)
        rc = self._lib.fr_server_tracks(self.h, ptr(metrics), ptr(clock), ptr(order), off.ctypes.data, T, n,
                                        int(max_attempts), int(buffer_size), float(retry_cooldown), float(det_gate),
                                        ptr(attempt), ptr(best), ptr(state), ptr(info), stream_of(self.device))
        if rc != FR_ERR_UNSUPPORTED or raise_on_track_error:
            check(rc, self.h)
        return attempt, best, state, info

    AGGREGATIONS = {"max": 0, "mean": 1, "topk": 2}

    def identity_scores(self, Q: torch.Tensor, E: torch.Tensor, offsets, aggregation: str = "mean", k: int = 3,
                        return_sim: bool = False):
        """The evaluation notebook's identity scores: probes ``Q`` f32 [n,512] against a multi-embedding
        gallery ``E`` f32 [G,512] on the device, identity i owning rows [offsets[i], offsets[i+1]) ->
        ``out`` f32 [n, n_ids] = the max, mean or top-k mean (``aggregation`` "max" / "mean" / "topk",
        ``k`` <= 16) of the probe's ``cosine_similarity`` against that identity's rows.  With
        ``return_sim`` also the f32 [n,G] similarity matrix: ``(out, sim)``.  The handle's own gallery
        is not touched."""
        if aggregation not in self.AGGREGATIONS:
            raise ValueError(f"aggregation must be one of {sorted(self.AGGREGATIONS)}")
        for name, x in (("Q", Q), ("E", E)):
            if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 512:
                raise ValueError(f"expected {name} as a float32 [rows,512] tensor")
            self._require_device(name, x)
        off, n_ids = _csr_offsets(offsets, E.shape[0], "offsets must name at least one identity and end at the "
                                  f"{E.shape[0]} rows of E", min_slices=1)
        Q, E = Q.contiguous(), E.contiguous()
        n, G = Q.shape[0], E.shape[0]
        out = torch.empty((n, n_ids), dtype=torch.float32, device=self.device)
        sim = torch.empty((n, G), dtype=torch.float32, device=self.device) if return_sim else None
        check(self._lib.fr_identity_scores(self.h, ptr(Q), n, ptr(E), off.ctypes.data, n_ids,
                                           self.AGGREGATIONS[aggregation], int(k), ptr(out), ptr(sim),
                                           stream_of(self.device)), self.h)
        return (out, sim) if return_sim else out

    # -- sample gallery / identity matching ---------------------------------
    def samples_set(self, E: torch.Tensor, offsets, tag=None) -> None:
        """The sample gallery of ``match_identities``: ``E`` f32 [G,512] (on the handle's device, or a
        host tensor), identity i owning rows [offsets[i], offsets[i+1]) (1..1024 rows each).  Replaces
        the previous one; no identities (``offsets`` of one entry) clears it.  The template gallery
        (``gallery_set`` / ``match``) is not touched."""
        if E.dtype != torch.float32 or E.dim() != 2 or (E.shape[0] and E.shape[1] != 512):
            raise ValueError("expected E as a float32 [rows,512] tensor")
        if E.device.type != "cpu":
            self._require_device("E", E)
        off, n_ids = _csr_offsets(offsets, E.shape[0], f"offsets must end at the {E.shape[0]} rows of E")
        E = E.contiguous()
        check(self._lib.fr_samples_set(self.h, ptr(E) if n_ids > 0 else None, off.ctypes.data, max(n_ids, 0),
                                       int(E.device.type != "cpu"), stream_of(self.device)), self.h)
        self.samples_tag = tag

    def samples_size(self):
        """(identities, rows) of the sample gallery; (0, 0) without one."""
        a, b = ctypes.c_int(), ctypes.c_int()
        check(self._lib.fr_samples_size(self.h, ctypes.byref(a), ctypes.byref(b)), self.h)
        return a.value, b.value

    def _identity_args(self, aggregation: str, agg_k: int, k: int, n: int, idx: torch.Tensor, score: torch.Tensor,
                       emb_out: Optional[torch.Tensor] = None) -> int:
        if aggregation not in self.AGGREGATIONS:
            raise ValueError(f"aggregation must be one of {sorted(self.AGGREGATIONS)}")
        k = int(k)
        if (idx.dtype != torch.int32 or score.dtype != torch.float32 or tuple(idx.shape) != (n, k)
                or tuple(score.shape) != (n, k) or not idx.is_contiguous() or not score.is_contiguous()):
            raise ValueError(f"idx / score must be contiguous int32 / float32 {[n, k]} tensors")
        self._require_device("idx / score", idx, score)
        if emb_out is not None:
            if emb_out.dtype != torch.float32 or tuple(emb_out.shape) != (n, 512) or not emb_out.is_contiguous():
                raise ValueError(f"emb_out must be a contiguous float32 {[n, 512]} tensor")
            self._require_device("emb_out", emb_out)
        return self.AGGREGATIONS[aggregation]

    def match_identities(self, Q: torch.Tensor, aggregation: str, agg_k: int, k: int, idx: torch.Tensor,
                         score: torch.Tensor) -> None:
        """The ``k`` best identities of every query of ``Q`` f32 [n,512] against the sample gallery ->
        ``idx`` int32 [n,k] (identity indices) / ``score`` f32 [n,k], descending, equal scores with the
        lower index first; the scores are ``identity_scores``' (``aggregation`` "max" / "mean" / "topk",
        ``agg_k`` <= 16 the top-k mean's k).  Asynchronous on the current stream."""
        if Q.dtype != torch.float32 or Q.dim() != 2 or Q.shape[1] != 512 or not Q.is_contiguous():
            raise ValueError("expected Q as a contiguous float32 [n,512] tensor")
        self._require_device("Q", Q)
        agg = self._identity_args(aggregation, agg_k, k, Q.shape[0], idx, score)
        check(self._lib.fr_match_identities(self.h, ptr(Q), Q.shape[0], agg, int(agg_k), int(k), ptr(idx), ptr(score),
                                            stream_of(self.device)), self.h)

    def embed_match_identities(self, rgb: torch.Tensor, aggregation: str, agg_k: int, k: int, idx: torch.Tensor,
                               score: torch.Tensor, emb_out: Optional[torch.Tensor] = None) -> None:
        """``embed_match`` with ``match_identities`` in place of the template match, in one library
        call: uint8 [n,112,112,3] crops -> idx / score [n,k] (and the normalised embeddings in
        ``emb_out`` f32 [n,512])."""
        agg = self._identity_args(aggregation, agg_k, k, rgb.shape[0], idx, score, emb_out)
        check(self._lib.fr_embed_match_identities(self.h, ptr(rgb), rgb.shape[0], agg, int(agg_k), int(k), ptr(idx),
                                                  ptr(score), ptr(emb_out), stream_of(self.device)), self.h)

    def eval_probes(self, scores: torch.Tensor, true_id: torch.Tensor, thresholds):
        """Per-probe records and threshold counts of a device score matrix ``scores`` f32 [n, n_ids]
        with the probes' true identity indices ``true_id`` int32 [n] (outside [0, n_ids): not
        enrolled) and up to 256 float64 ``thresholds`` -> (rec_i int32 [n,4] = predicted, best, rank,
        has_impostor; rec_f f32 [n,4] = best score, genuine, impostor, 0; counts int64 [T,4] = tp, fp,
        fn, genuine >= threshold) on the device (include/frhip.h: fr_eval_probes)."""
        import numpy as np
        if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[1] < 1:
            raise ValueError("expected scores as a float32 [n, n_ids] tensor with n_ids >= 1")
        if true_id.dtype != torch.int32 or tuple(true_id.shape) != (scores.shape[0],):
            raise ValueError("expected true_id as an int32 [n] tensor")
        for name, x in (("scores", scores), ("true_id", true_id)):
            self._require_device(name, x)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        if thr.shape[0] > 256:
            raise ValueError("at most 256 thresholds per call")
        scores, true_id = scores.contiguous(), true_id.contiguous()
        n, T = scores.shape[0], thr.shape[0]
        rec_i = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        rec_f = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        counts = torch.empty((T, 4), dtype=torch.int64, device=self.device)
        check(self._lib.fr_eval_probes(self.h, ptr(scores), n, scores.shape[1], ptr(true_id),
                                       thr.ctypes.data if T else None, T, ptr(rec_i), ptr(rec_f),
                                       ptr(counts) if T else None, stream_of(self.device)), self.h)
        return rec_i, rec_f, counts

    # -- alignment / quality ----------------------------------------------
    def align_faces(self, frame: torch.Tensor, landmarks, out_size: int, out: torch.Tensor):
        """frame: uint8 [H,W,3] on device; landmarks: host float32 [n,5,2] -> out [n,S,S,3]; returns tforms."""
        import numpy as np
        lm = np.ascontiguousarray(landmarks, dtype=np.float32)
        n = lm.shape[0]
        tf = np.empty((n, 2, 3), dtype=np.float64)
        check(self._lib.fr_align_faces(self.h, ptr(frame), frame.shape[0], frame.shape[1], lm.ctypes.data, n,
                                       int(out_size), ptr(out), tf.ctypes.data, stream_of(self.device)), self.h)
        return tf

    def warp_affine(self, frame: torch.Tensor, tforms, out_size: int, out: torch.Tensor) -> None:
        import numpy as np
        tf = np.ascontiguousarray(tforms, dtype=np.float64)
        check(self._lib.fr_warp_affine(self.h, ptr(frame), frame.shape[0], frame.shape[1], tf.ctypes.data,
                                       tf.shape[0], int(out_size), ptr(out), stream_of(self.device)), self.h)

    def blur_scores(self, crops: torch.Tensor):
        """uint8 [n,H,W] (gray) or [n,H,W,C] (C = 3 / 4, RGB(A)) on the device -> float64 [n]."""
        import numpy as np
        if crops.dtype != torch.uint8 or crops.dim() not in (3, 4):
            raise ValueError("expected uint8 [n,H,W] or [n,H,W,C] images")
        n = crops.shape[0]
        c = 1 if crops.dim() == 3 else crops.shape[3]
        out = np.empty(n, dtype=np.float64)
        check(self._lib.fr_blur_scores(self.h, ptr(crops), n, crops.shape[1], crops.shape[2], c, out.ctypes.data,
                                       stream_of(self.device)), self.h)
        return out

    # -- detector (arch "scrfd_10g") ---------------------------------------
    def detect(self, frames: torch.Tensor, det_thresh: float = 0.5, max_faces: int = 256):
        """frames: uint8 [n,H,W,3] RGB on the device -> (dets f32 [n,max_faces,15], counts int32 [n]);
        row i < min(counts[f], max_faces) of frame f = x1 y1 x2 y2 score, 5 x (x, y)."""
        import numpy as np
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("expected uint8 [n,H,W,3] RGB frames")
        frames = frames.to(self.device).contiguous()
        n = frames.shape[0]
        dets = np.zeros((n, max_faces, 15), dtype=np.float32)
        counts = np.zeros(n, dtype=np.int32)
        check(self._lib.fr_detect(self.h, ptr(frames), n, frames.shape[1], frames.shape[2], float(det_thresh),
                                  int(max_faces), dets.ctypes.data, counts.ctypes.data, stream_of(self.device)),
              self.h)
        return dets, counts

    # -- the chain with device outputs (asynchronous on the current stream, capturable) ------
    def _out(self, name: str, t, shape, dtype, zero: bool = False) -> torch.Tensor:
        """The caller's output tensor ``t`` checked, or a new one."""
        if t is None:
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} {list(shape)} tensor on {self.device}")
        return t

    def _frames(self, frames: torch.Tensor) -> torch.Tensor:
        if (not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4
                or frames.shape[3] != 3):
            raise ValueError("expected uint8 [n,H,W,3] RGB frames")
        self._require_device("frames", frames)
        return frames.contiguous()

    def detect_device(self, frames: torch.Tensor, det_thresh: float = 0.5, max_faces: int = 256, dets=None,
                      counts=None):
        """``detect`` with device outputs and no synchronisation (fr_detect_device): frames uint8
        [n,H,W,3] on the device -> (dets f32 [n,max_faces,15], counts int32 [n]) on the device; rows
        i < min(counts[f], max_faces) are ``detect``'s, ``counts[f] == -1`` marks a frame over the
        4096-candidate limit (where ``detect`` raises).  ``dets`` / ``counts``: tensors to write
        (for graph capture); new ``dets`` are zero-filled."""
        frames = self._frames(frames)
        n, F = frames.shape[0], int(max_faces)
        dets = self._out("dets", dets, (n, F, 15), torch.float32, zero=True)
        counts = self._out("counts", counts, (n,), torch.int32)
        check(self._lib.fr_detect_device(self.h, ptr(frames), n, frames.shape[1], frames.shape[2], float(det_thresh),
                                         F, ptr(dets) if F else None, ptr(counts), stream_of(self.device)), self.h)
        return dets, counts

    def align_device(self, frames: torch.Tensor, landmarks: torch.Tensor, counts, out_size: int, out=None,
                     tforms=None, ok=None):
        """``align_faces`` for every slot of a batch of frames, landmarks read on the device, no
        synchronisation (fr_align_device).  frames uint8 [n,H,W,3]; ``landmarks`` float32 on the
        device, either detection rows [n,F,15] (``detect_device``'s dets, read in place) or
        [n,F,5,2]; ``counts`` int32 [n] on the device (slots i < min(counts[f], F) are live) or None
        (all live) -> (crops uint8 [n,F,S,S,3], tforms f64 [n,F,2,3], ok uint8 [n,F]).  A slot with
        ok == 0 (not live, or a fit the host refuses) has an all-zero crop and a NaN tform."""
        frames = self._frames(frames)
        n, S = frames.shape[0], int(out_size)
        lm = landmarks
        if (not isinstance(lm, torch.Tensor) or lm.dtype != torch.float32 or lm.dim() not in (3, 4)
                or lm.shape[0] != n or tuple(lm.shape[2:]) not in ((15,), (5, 2))):
            raise ValueError(f"landmarks must be float32 [{n},F,15] detection rows or [{n},F,5,2]")
        self._require_device("landmarks", lm)
        lm = lm.contiguous()
        F = lm.shape[1]
        rows = lm.dim() == 3
        if counts is not None:
            if counts.dtype != torch.int32 or tuple(counts.shape) != (n,) or not counts.is_contiguous():
                raise ValueError(f"counts must be a contiguous int32 [{n}] tensor")
            self._require_device("counts", counts)
        out = self._out("out", out, (n, F, S, S, 3), torch.uint8)
        tforms = self._out("tforms", tforms, (n, F, 2, 3), torch.float64)
        ok = self._out("ok", ok, (n, F), torch.uint8)
        lm_ptr = (ptr(lm) + (5 * 4 if rows else 0)) if n * F else None
        check(self._lib.fr_align_device(self.h, ptr(frames), n, frames.shape[1], frames.shape[2], lm_ptr,
                                        15 if rows else 10, ptr(counts), F, S, ptr(out), ptr(tforms), ptr(ok),
                                        stream_of(self.device)), self.h)
        return out, tforms, ok

    def blur_scores_device(self, crops: torch.Tensor, out=None) -> torch.Tensor:
        """``blur_scores`` with the float64 [n] result on the device and no synchronisation."""
        if crops.dtype != torch.uint8 or crops.dim() not in (3, 4):
            raise ValueError("expected uint8 [n,H,W] or [n,H,W,C] images")
        self._require_device("crops", crops)
        crops = crops.contiguous()
        n = crops.shape[0]
        c = 1 if crops.dim() == 3 else crops.shape[3]
        out = self._out("out", out, (n,), torch.float64)
        check(self._lib.fr_blur_scores_device(self.h, ptr(crops), n, crops.shape[1], crops.shape[2], c, ptr(out),
                                              stream_of(self.device)), self.h)
        return out

    def quality_gate_device(self, dets: torch.Tensor, counts, ok, blur, config, out=None):
        """The quality gate, the per-frame order and the packed face lists on the device, no
        synchronisation (fr_quality_gate_device).  dets float32 [n,F,15]; counts int32 [n] or None;
        ok uint8 [n,F] or None; blur float64 with n * F elements or None; ``config``: the seven
        fields of fr_gate_config by name -> a dict of the device tensors ``GATE_OUTPUTS``: stage uint8
        [n,F], metrics f64 [n,F,5], bbox int32 [n,F,4], rank int32 [n,F], rows int32 [n*F],
        frame_offsets int32 [n+1], valid_slots int32 [n*F], n_valid int32 [1].  ``out``: such a dict
        to write again (for graph capture)."""
        if (not isinstance(dets, torch.Tensor) or dets.dtype != torch.float32 or dets.dim() != 3
                or dets.shape[2] != 15):
            raise ValueError("dets must be float32 [n,F,15] detection rows")
        self._require_device("dets", dets)
        dets = dets.contiguous()
        n, F = dets.shape[0], dets.shape[1]
        for name, t, dtype, numel in (("counts", counts, torch.int32, n), ("ok", ok, torch.uint8, n * F),
                                      ("blur", blur, torch.float64, n * F)):
            if t is not None:
                if t.dtype != dtype or t.numel() != numel or not t.is_contiguous():
                    raise ValueError(f"{name} must be a contiguous {dtype} tensor of {numel} elements")
                self._require_device(name, t)
        shapes = {"stage": ((n, F), torch.uint8), "metrics": ((n, F, 5), torch.float64),
                  "bbox": ((n, F, 4), torch.int32), "rank": ((n, F), torch.int32), "rows": ((n * F,), torch.int32),
                  "frame_offsets": ((n + 1,), torch.int32), "valid_slots": ((n * F,), torch.int32),
                  "n_valid": ((1,), torch.int32)}
        o = {k: self._out(k, None if out is None else out.get(k), *shapes[k], zero=(n == 0)) for k in GATE_OUTPUTS}
        cfg = GateConfig(**{k: config[k] for k, _ in GateConfig._fields_})
        check(self._lib.fr_quality_gate_device(self.h, ptr(dets), ptr(counts), ptr(ok), ptr(blur), n, F,
                                               ctypes.byref(cfg), *(ptr(o[k]) for k in GATE_OUTPUTS),
                                               stream_of(self.device)), self.h)
        return o

    def _image_list(self, images):
        """A list of uint8 [H,W,3] device tensors -> (contiguous tensors on the handle's device, host
        pointer array uint64 [n], host sizes int32 [n,2]) as fr_detect_images / fr_align_images take them."""
        import numpy as np
        kept = []
        for i, im in enumerate(images):
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                raise ValueError(f"image {i}: expected a uint8 [H,W,3] RGB tensor")
            kept.append(im.to(self.device).contiguous())
        ptrs = np.array([im.data_ptr() if im.numel() else 0 for im in kept], dtype=np.uint64)
        sizes = np.array([[im.shape[0], im.shape[1]] for im in kept], dtype=np.int32).reshape(-1, 2)
        return kept, ptrs, sizes

    def detect_images(self, images, det_thresh: float = 0.5, max_faces: int = 256):
        """``detect`` for a list of uint8 [H,W,3] RGB device tensors of different sizes, in one call
        (chunks of the handle's max_frames, per-image letterbox geometry: include/frhip.h,
        fr_detect_images) -> (dets f32 [n,max_faces,15], counts int32 [n]), rows as ``detect`` gives them."""
        import numpy as np
        kept, ptrs, sizes = self._image_list(images)
        n = len(kept)
        dets = np.zeros((n, max(int(max_faces), 0), 15), dtype=np.float32)
        counts = np.zeros(n, dtype=np.int32)
        check(self._lib.fr_detect_images(self.h, ptrs.ctypes.data, sizes.ctypes.data, n, float(det_thresh),
                                         int(max_faces), dets.ctypes.data, counts.ctypes.data,
                                         stream_of(self.device)), self.h)
        return dets, counts

    def align_images(self, images, landmarks, face_image, out_size: int, out: torch.Tensor):
        """``align_faces`` for faces of different images: ``images`` a list of uint8 [H,W,3] device
        tensors, ``landmarks`` host float32 [n,5,2], ``face_image`` int32 [n] (the image of each face)
        -> out uint8 [n,S,S,3] on the device, in one launch; returns tforms float64 [n,2,3]."""
        import numpy as np
        kept, ptrs, sizes = self._image_list(images)
        lm = np.ascontiguousarray(landmarks, dtype=np.float32).reshape(-1, 5, 2)
        fi = np.ascontiguousarray(face_image, dtype=np.int32).reshape(-1)
        n = lm.shape[0]
        if fi.shape[0] != n:
            raise ValueError(f"face_image names {fi.shape[0]} faces, landmarks {n}")
        S = int(out_size)
        if (out.dtype != torch.uint8 or tuple(out.shape) != (n, S, S, 3) or out.device != self.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 {[n, S, S, 3]} tensor on {self.device}")
        tf = np.empty((n, 2, 3), dtype=np.float64)
        check(self._lib.fr_align_images(self.h, ptrs.ctypes.data, sizes.ctypes.data, len(kept), lm.ctypes.data,
                                        fi.ctypes.data, n, S, ptr(out) if n else None, tf.ctypes.data,
                                        stream_of(self.device)), self.h)
        return tf

    def detect_images_device(self, images, det_thresh: float = 0.5, max_faces: int = 256, dets=None, counts=None):
        """``detect_images`` with device outputs and no synchronisation (fr_detect_images_device): a
        list of uint8 [H,W,3] RGB device tensors of different sizes -> (dets f32 [n,max_faces,15],
        counts int32 [n]) on the device; rows i < min(counts[f], max_faces) are ``detect_images``',
        ``counts[f] == -1`` marks an image over the 4096-candidate limit (where ``detect_images``
        raises).  The resize tables are made on the device and the geometry travels in the kernel
        arguments: nothing is staged.  ``dets`` / ``counts``: tensors to write; new ``dets`` are
        zero-filled.  The images must stay alive until the stream has run the call."""
        images = list(images)
        for i, im in enumerate(images):
            if isinstance(im, torch.Tensor):
                self._require_device(f"image {i}", im)
        kept, ptrs, sizes = self._image_list(images)
        n, F = len(kept), max(int(max_faces), 0)
        dets = self._out("dets", dets, (n, F, 15), torch.float32, zero=True)
        counts = self._out("counts", counts, (n,), torch.int32)
        check(self._lib.fr_detect_images_device(self.h, ptrs.ctypes.data, sizes.ctypes.data, n, float(det_thresh),
                                                int(max_faces), ptr(dets) if n * F else None, ptr(counts),
                                                stream_of(self.device)), self.h)
        return dets, counts

    def align_images_device(self, images, landmarks: torch.Tensor, counts, out_size: int, out=None, tforms=None,
                            ok=None):
        """``align_device`` with a source per image (fr_align_images_device): ``images`` a list of n
        uint8 [H,W,3] device tensors of different sizes; ``landmarks`` float32 on the device, detection
        rows [n,F,15] (read in place) or [n,F,5,2]; ``counts`` int32 [n] on the device or None (all
        live) -> (crops uint8 [n,F,S,S,3], tforms f64 [n,F,2,3], ok uint8 [n,F]).  Slot (i, k) warps
        image i; a slot with ok == 0 has an all-zero crop and a NaN tform.  No synchronisation."""
        images = list(images)
        for i, im in enumerate(images):
            if isinstance(im, torch.Tensor):
                self._require_device(f"image {i}", im)
        kept, ptrs, sizes = self._image_list(images)
        n, S = len(kept), int(out_size)
        lm = landmarks
        if (not isinstance(lm, torch.Tensor) or lm.dtype != torch.float32 or lm.dim() not in (3, 4)
                or lm.shape[0] != n or tuple(lm.shape[2:]) not in ((15,), (5, 2))):
            raise ValueError(f"landmarks must be float32 [{n},F,15] detection rows or [{n},F,5,2]")
        self._require_device("landmarks", lm)
        lm = lm.contiguous()
        F = lm.shape[1]
        rows = lm.dim() == 3
        if counts is not None:
            if counts.dtype != torch.int32 or tuple(counts.shape) != (n,) or not counts.is_contiguous():
                raise ValueError(f"counts must be a contiguous int32 [{n}] tensor")
            self._require_device("counts", counts)
        out = self._out("out", out, (n, F, S, S, 3), torch.uint8)
        tforms = self._out("tforms", tforms, (n, F, 2, 3), torch.float64)
        ok = self._out("ok", ok, (n, F), torch.uint8)
        lm_ptr = (ptr(lm) + (5 * 4 if rows else 0)) if n * F else None
        check(self._lib.fr_align_images_device(self.h, ptrs.ctypes.data, sizes.ctypes.data, n, lm_ptr,
                                               15 if rows else 10, ptr(counts), F, S, ptr(out), ptr(tforms), ptr(ok),
                                               stream_of(self.device)), self.h)
        return out, tforms, ok

    def resize_images(self, images, out: torch.Tensor) -> None:
        """``resize_crops`` for a list of uint8 [H,W,3] RGB device tensors of different sizes -> out uint8
        [n,112,112,3] on the device, one launch per chunk of the handle's max_batch (include/frhip.h,
        fr_resize_images)."""
        kept, ptrs, sizes = self._image_list(images)
        n = len(kept)
        if (out.dtype != torch.uint8 or tuple(out.shape) != (n, 112, 112, 3) or out.device != self.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 {[n, 112, 112, 3]} tensor on {self.device}")
        check(self._lib.fr_resize_images(self.h, ptrs.ctypes.data, sizes.ctypes.data, n, ptr(out) if n else None,
                                         stream_of(self.device)), self.h)

    def embed_images(self, images, out: torch.Tensor, normalize: bool = True) -> None:
        """``embed`` for such a list -> out float32 [n,512] on the device, in fr_embed's chunks of
        max_batch, each resized straight into the forward's input (fr_embed_images)."""
        _kept, ptrs, sizes = self._image_list(images)
        self.embed_image_ptrs(ptrs, sizes, out, normalize)

    def embed_image_ptrs(self, ptrs, sizes, out: torch.Tensor, normalize: bool = True) -> None:
        """``embed_images`` on the arrays the library takes: ``ptrs`` uint64 [n] device addresses of
        uint8 [h_i, w_i, 3] images, ``sizes`` int32 [n,2] = h_i, w_i (a caller that packed many crops into
        one allocation passes addresses inside it).  The images must stay allocated until the current
        stream has run the call."""
        import numpy as np
        ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64).reshape(-1)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 2)
        n = ptrs.shape[0]
        if sizes.shape[0] != n:
            raise ValueError(f"sizes names {sizes.shape[0]} images, ptrs {n}")
        if (out.dtype != torch.float32 or tuple(out.shape) != (n, 512) or out.device != self.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 {[n, 512]} tensor on {self.device}")
        check(self._lib.fr_embed_images(self.h, ptrs.ctypes.data, sizes.ctypes.data, n, ptr(out) if n else None,
                                        int(normalize), stream_of(self.device)), self.h)

    def set_precision(self, mode: str) -> None:
        modes = {"fp32": 0, "f32": 0, "bf16x3": 1}
        if mode not in modes:
            raise ValueError(f"precision must be one of {sorted(modes)}")
        check(self._lib.fr_set_precision(self.h, modes[mode]), self.h)

    def set_conv_algorithm(self, algo: str) -> None:
        algos = {"direct": 0, "winograd": 1, "winograd4": 2}
        if algo not in algos:
            raise ValueError(f"conv_algorithm must be one of {sorted(algos)}")
        check(self._lib.fr_set_conv_algorithm(self.h, algos[algo]), self.h)

    def set_graph_batch(self, max_n: int) -> None:
        """Replay forwards of n <= max_n crops as captured hipGraphs (0 disables)."""
        check(self._lib.fr_set_graph_batch(self.h, int(max_n)), self.h)

    def set_lanes(self, min_n: int, max_lanes: int = 2) -> None:
        """Run a forward of n crops as min(max_lanes, n // min_n) concurrent parts (0: one lane)."""
        check(self._lib.fr_set_lanes(self.h, int(min_n), int(max_lanes)), self.h)

    def get_lanes(self) -> dict:
        """The lane setting in force; ``fell_back`` is True when a failed workspace allocation
        turned lanes off (until the next ``set_lanes``)."""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(self._lib.fr_get_lanes(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), self.h)
        return {"min_n": a.value, "max_lanes": b.value, "fell_back": bool(c.value)}

    def graph_count(self) -> int:
        c = ctypes.c_int()
        check(self._lib.fr_graph_count(self.h, ctypes.byref(c)), self.h)
        return c.value

    # -- profiling ---------------------------------------------------------
    def profile_enable(self, on: bool = True) -> None:
        check(self._lib.fr_profile_enable(self.h, int(on)), self.h)

    def profile_read(self) -> dict:
        cms, cfl, tms = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        cn = ctypes.c_int64()
        check(self._lib.fr_profile_read(self.h, ctypes.byref(cms), ctypes.byref(cfl), ctypes.byref(cn),
                                        ctypes.byref(tms)), self.h)
        out = {"conv_ms": cms.value, "conv_flop": cfl.value, "conv_launches": cn.value, "total_ms": tms.value}
        for kind, name in ((0, "other"), (1, "direct"), (2, "winograd")):
            ms, fl, ex = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            n = ctypes.c_int64()
            check(self._lib.fr_profile_kernel(self.h, kind, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(ex),
                                              ctypes.byref(n)), self.h)
            out[name] = {"ms": ms.value, "flop": fl.value, "exec_flop": ex.value, "launches": n.value}
        return out
