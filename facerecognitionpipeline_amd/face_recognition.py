"""Drop-in ``FaceAligner`` / ``FaceQualityFilter`` / ``FaceProcessor`` (face_recognition.py:50-216).

Alignment (cv2.estimateAffinePartial2D + cv2.warpAffine, face_recognition.py:64-74)
and the blur score (cv2.Laplacian variance, :94-99) run on the GPU through
``fr_align_faces`` / ``fr_warp_affine`` / ``fr_blur_scores``, so a frame uploaded
once yields crops that stay in HBM for ``FaceEmbedder.embed_tensor``.  Pose
angles and the threshold logic are scalar host code, as in the reference.

``FaceDetector`` replaces insightface ``FaceAnalysis('buffalo_l')`` (SCRFD
det_10g, :19-48) with the SCRFD-10G network on the GPU (``fr_detect``:
letterbox, MFMA conv pyramid, anchor decode, NMS).  No weights exist offline,
so it runs seeded synthetic weights unless ``model_path`` / ``state_dict``
gives a state dict in ``detector_arch`` keys; ``FaceProcessor`` also accepts
any detector object with the reference's
``detect(image_rgb) -> [{'bbox','landmarks','det_score',...}]`` contract.

Images of different sizes (a folder of photographs) go through ``detect_images`` /
``align_images`` / ``FaceProcessor.process_images``: one detect call, one align launch and
one blur call for the whole sequence (``fr_detect_images`` / ``fr_align_images``), per image
the single-image arithmetic.  ``process_images(gate="device")`` keeps that pass in HBM
(``device_chain_images``: ``fr_detect_images_device`` / ``fr_align_images_device``).

Parity of the OpenCV arithmetic is UNPINNED (cv2 absent); the kernels are
pinned bit-exactly to the restatement in ``oracle/align_ref.py``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib


def reference_template(output_size: int) -> np.ndarray:
    S = output_size
    return np.array([[0.34 * S, 0.46 * S], [0.66 * S, 0.46 * S], [0.50 * S, 0.61 * S],
                     [0.37 * S, 0.74 * S], [0.63 * S, 0.74 * S]], dtype=np.float32)


class _DeviceOps:
    """One lightweight handle for the alignment / quality kernels (no model weights)."""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._h: Optional[_lib.Handle] = None

    @property
    def handle(self) -> "_lib.Handle":
        if self._h is None:
            self._h = _lib.Handle("ir_50", "adaface", self.device, max_batch=1)
        return self._h


class FaceAligner:
    def __init__(self, output_size: int = 112, device=None):
        self.output_size = output_size
        self.template = reference_template(output_size)
        self._ops = _DeviceOps(device)

    def align(self, image: np.ndarray, landmarks: np.ndarray, method: str = "similarity") -> np.ndarray:
        """Host image in, host crop out (reference signature).  A 2-D gray image gives a 2-D crop,
        as cv2.warpAffine does (each channel of the warp is the single-channel warp)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        gray = img.ndim == 2
        if gray:
            img = np.repeat(img[:, :, None], 3, axis=2)
        frame = torch.from_numpy(img).to(self._ops.device)
        out = self.align_batch(frame, np.asarray(landmarks, np.float32)[None], method)[0].cpu().numpy()
        return np.ascontiguousarray(out[..., 0]) if gray else out

    def align_batch(self, frame: torch.Tensor, landmarks: np.ndarray, method: str = "similarity") -> torch.Tensor:
        """Device form: uint8 [H,W,3] frame on the GPU, float32 [n,5,2] landmarks -> uint8 [n,S,S,3] on the GPU."""
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise ValueError("expected a uint8 [H,W,3] RGB frame tensor")
        lm = np.ascontiguousarray(landmarks, dtype=np.float32).reshape(-1, 5, 2)
        S = self.output_size
        out = torch.empty((lm.shape[0], S, S, 3), dtype=torch.uint8, device=self._ops.device)
        frame = frame.to(self._ops.device).contiguous()
        if method == "similarity":
            self._ops.handle.align_faces(frame, lm, S, out)
        else:
            tf = np.stack([affine_from_3_points(x[:3], self.template[:3]) for x in lm])
            self._ops.handle.warp_affine(frame, tf, S, out)
        return out

    def align_images(self, images, landmarks_per_image, method: str = "similarity") -> torch.Tensor:
        """``align_batch`` over images of different sizes in one launch: ``images`` a sequence of uint8
        [H,W,3] frames (host arrays or device tensors), ``landmarks_per_image[i]`` the float32 [k_i,5,2]
        landmarks of image i's faces (k_i may be 0) -> uint8 [sum k_i,S,S,3] on the GPU, image by image
        in face order.  Any ``method`` but "similarity" runs ``align_batch`` per image."""
        if len(images) != len(landmarks_per_image):
            raise ValueError(f"{len(images)} images but landmarks for {len(landmarks_per_image)}")
        dev, S = self._ops.device, self.output_size
        frames = [_device_frame(im, dev) for im in images]
        lms = [np.ascontiguousarray(lm, dtype=np.float32).reshape(-1, 5, 2) for lm in landmarks_per_image]
        total = sum(lm.shape[0] for lm in lms)
        if method != "similarity":
            parts = [self.align_batch(f, lm, method) for f, lm in zip(frames, lms) if lm.shape[0]]
            return torch.cat(parts) if parts else torch.empty((0, S, S, 3), dtype=torch.uint8, device=dev)
        out = torch.empty((total, S, S, 3), dtype=torch.uint8, device=dev)
        if total:
            face_image = np.repeat(np.arange(len(lms), dtype=np.int32), [lm.shape[0] for lm in lms])
            self._ops.handle.align_images(frames, np.concatenate(lms), face_image, S, out)
        return out


def _device_frame(image, device) -> torch.Tensor:
    """A host array or device tensor, uint8 [H,W,3] or gray [H,W] (replicated to three channels, as
    cv2.COLOR_GRAY2BGR does), as a contiguous uint8 [H,W,3] tensor on ``device``."""
    if isinstance(image, torch.Tensor):
        t = image
        if t.dim() == 2:
            t = t[:, :, None].expand(-1, -1, 3)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"expected a uint8 HxW or HxWx3 image, got {t.dtype} {tuple(t.shape)}")
        return t.to(device).contiguous()
    return torch.from_numpy(FaceDetector._to_rgb(np.asarray(image))).to(device)


def affine_from_3_points(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """cv2.getAffineTransform(src[:3], dst[:3]) (exact 3-point solve, float64)."""
    s = np.asarray(src, np.float32).astype(np.float64)
    d = np.asarray(dst, np.float32).astype(np.float64)
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        A[2 * i, :3] = [s[i, 0], s[i, 1], 1.0]
        A[2 * i + 1, 3:] = [s[i, 0], s[i, 1], 1.0]
        b[2 * i], b[2 * i + 1] = d[i, 0], d[i, 1]
    return np.linalg.solve(A, b).reshape(2, 3)


class FaceQualityFilter:
    def __init__(self, min_det_score=0.6, min_face_size=60, max_yaw=45, max_pitch=30, max_roll=30,
                 check_blur=True, blur_threshold=100, device=None):
        self.min_det_score = min_det_score
        self.min_face_size = min_face_size
        self.max_yaw = max_yaw
        self.max_pitch = max_pitch
        self.max_roll = max_roll
        self.check_blur = check_blur
        self.blur_threshold = blur_threshold
        self._ops = _DeviceOps(device)

    def compute_blur_score(self, face_image) -> float:
        """cv2.Laplacian(gray, CV_64F).var() of one image (face_recognition.py:94-99): a 3-D
        [H,W,3] (or [H,W,4]) RGB image goes through RGB2GRAY, a 2-D one is the gray image.  Any
        size.  Returns np.float64, like ndarray.var() in the reference."""
        t = face_image if isinstance(face_image, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(face_image, np.uint8))
        if t.dim() not in (2, 3):
            raise ValueError(f"expected an HxW or HxWxC image, got {tuple(t.shape)}")
        return np.float64(self.compute_blur_scores(t.unsqueeze(0))[0])

    def compute_blur_scores(self, crops) -> np.ndarray:
        """A batch of one size (host array or device tensor): uint8 [n,H,W,3|4] RGB(A) or
        [n,H,W] gray -> float64 [n]."""
        t = crops if isinstance(crops, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(crops, np.uint8))
        if t.dtype != torch.uint8:
            t = t.to(torch.uint8)
        if t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[3] not in (1, 3, 4)):
            raise ValueError(f"expected uint8 [n,H,W] gray or [n,H,W,3] RGB images, got {tuple(t.shape)}")
        if t.dim() == 4 and t.shape[3] == 1:
            t = t[..., 0]
        return self._ops.handle.blur_scores(t.to(self._ops.device).contiguous())

    def compute_pose_angles(self, landmarks: np.ndarray) -> Dict[str, float]:
        le, re, nose, lm, rm = [np.asarray(p) for p in landmarks]
        eye_c = (le + re) / 2
        d = re - le
        roll = np.degrees(np.arctan2(d[1], d[0]))
        yaw = np.degrees(np.arcsin(np.clip((nose[0] - eye_c[0]) / np.linalg.norm(d), -1, 1))) * 2
        mouth_c = (lm + rm) / 2
        pitch = ((nose[1] - eye_c[1]) / (mouth_c[1] - eye_c[1]) - 0.5) * 60
        return {"yaw": yaw, "pitch": pitch, "roll": roll}

    def is_valid(self, face_dict: Dict, face_image=None, blur_score: Optional[float] = None) -> Tuple[bool, Dict]:
        m: Dict = {"det_score": face_dict["det_score"]}
        if m["det_score"] < self.min_det_score:
            return False, m
        x0, y0, x1, y1 = face_dict["bbox"][:4]
        m["face_size"] = min(x1 - x0, y1 - y0)
        if m["face_size"] < self.min_face_size:
            return False, m
        pose = self.compute_pose_angles(face_dict["landmarks"])
        m.update(pose)
        if abs(pose["yaw"]) > self.max_yaw or abs(pose["pitch"]) > self.max_pitch or abs(pose["roll"]) > self.max_roll:
            return False, m
        if self.check_blur and (face_image is not None or blur_score is not None):
            m["blur_score"] = np.float64(blur_score) if blur_score is not None else self.compute_blur_score(face_image)
            if m["blur_score"] < self.blur_threshold:
                return False, m
        return True, m

    def gate_device(self, dets: torch.Tensor, counts, ok=None, blur=None, out: Optional[Dict] = None) -> Dict:
        """``is_valid`` for every slot of a batch of frames, ``process_numpy``'s order per frame and the
        packed face lists, on the device and without a synchronisation (``fr_quality_gate_device``):
        dets float32 [n,F,15] (``detect_device``), counts int32 [n] or None, ok uint8 [n,F]
        (``align_device``) or None, blur float64 [n,F] or [n*F] (``blur_scores_device``) or None ->
        a dict of device tensors: stage uint8 [n,F] (``GATE_*``), metrics float64 [n,F,5] (det_score,
        blur_score, yaw, pitch, roll), bbox int32 [n,F,4], rank int32 [n,F], rows int32 [n*F],
        frame_offsets int32 [n+1], valid_slots int32 [n*F], n_valid int32 [1].  ``out``: a dict from
        an earlier call whose tensors are written again (for graph capture).  The values are
        ``quality_gate_host``'s; what that means against ``is_valid`` is stated there."""
        return self._ops.handle.quality_gate_device(dets, counts, ok, blur, _gate_config(self), out)

    def metrics_from_gate(self, stage, metrics_row, bbox_row, blur_checked: Optional[bool] = None) -> Dict:
        """The ``quality_metrics`` dict ``is_valid`` returns, rebuilt from one slot of the gate's
        outputs: the same keys in the same insertion order for that stage (the early exit) and the
        same types -- det_score a Python float, face_size np.int32, the angles np.float32, blur_score
        np.float64.  ``blur_checked``: whether the gate ran its blur test (default: ``check_blur``;
        False for a gate that ran without blur scores)."""
        stage = int(stage)
        if stage == GATE_NOT_LIVE:
            raise ValueError("the slot is not live")
        m: Dict = {"det_score": float(metrics_row[0])}
        if stage == GATE_DET_SCORE:
            return m
        b = np.asarray(bbox_row, np.int32)
        m["face_size"] = min(b[2] - b[0], b[3] - b[1])
        if stage == GATE_FACE_SIZE:
            return m
        m["yaw"], m["pitch"], m["roll"] = (np.float32(metrics_row[k]) for k in (2, 3, 4))
        if stage == GATE_POSE:
            return m
        if self.check_blur if blur_checked is None else blur_checked:
            m["blur_score"] = np.float64(metrics_row[1])
        return m


GATE_MAX_FACES = 1024  # FR_GATE_MAX_FACES
GATE_VALID, GATE_DET_SCORE, GATE_FACE_SIZE, GATE_POSE, GATE_BLUR, GATE_FIT, GATE_NOT_LIVE = 0, 1, 2, 3, 4, 5, 255
_GATE_CONFIG_KEYS = ("min_det_score", "min_face_size", "max_yaw", "max_pitch", "max_roll", "blur_threshold")


def _gate_config(config) -> Dict:
    """A ``FaceQualityFilter`` or a dict of its constructor arguments -> the seven fields of
    ``fr_gate_config``; ``ValueError`` for a limit that is not finite or lies beyond +-FLT_MAX."""
    if isinstance(config, FaceQualityFilter):
        c = {k: getattr(config, k) for k in _GATE_CONFIG_KEYS + ("check_blur",)}
    else:
        c = dict(min_det_score=0.6, min_face_size=60, max_yaw=45, max_pitch=30, max_roll=30, check_blur=True,
                 blur_threshold=100)
        c.update(config or {})
    out = {k: float(c[k]) for k in _GATE_CONFIG_KEYS}
    fmax = float(np.finfo(np.float32).max)
    for k, v in out.items():
        if not -fmax <= v <= fmax:  # a NaN fails both
            raise ValueError(f"{k} = {v} is not finite or lies beyond +-FLT_MAX")
    out["check_blur"] = bool(c["check_blur"])
    return out


def quality_gate_host(dets, counts, ok, blur, config, max_faces: Optional[int] = None):
    """The contract of ``fr_quality_gate_device`` (include/frhip.h) in vectorised numpy: the gate of
    ``FaceQualityFilter.is_valid`` per slot, the order of ``process_numpy`` per frame and the packed
    face lists, for dets float32 [n,F,15] (x0 y0 x1 y1 score, 5 x (x, y)), counts int32 [n] or None
    (every slot live), ok uint8 [n,F] or None, blur float64 [n,F] or None; ``config`` a
    ``FaceQualityFilter`` or a dict of its arguments.

    -> (stage uint8 [n,F], metrics float64 [n,F,5] = det_score, blur_score, yaw, pitch, roll,
    bbox int32 [n,F,4], rank int32 [n,F], rows int32 [n*F], frame_offsets int32 [n+1],
    valid_slots int32 [n*F], n_valid int32 [1]).

    Everything is float32 / float64 IEEE arithmetic as ``is_valid`` does it, except that arctan2 and
    arcsin are taken in double and rounded to float32: numpy's own float32 forms are a few ulp off
    the correctly rounded value and differ between hosts, so the contract names the value they
    approximate.  Against ``is_valid`` on any numpy: pitch and everything else bitwise, yaw and roll
    within 1e-4 degrees (yaw for |ratio| <= 0.95), the decision equal unless an angle lies that close
    to its limit."""
    d = np.ascontiguousarray(dets, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 15:
        raise ValueError("dets must be float32 [n,F,15] detection rows")
    n, F = d.shape[0], d.shape[1]
    if max_faces is not None and int(max_faces) != F:
        raise ValueError(f"dets have {F} slots per frame, max_faces is {max_faces}")
    if not 1 <= F <= GATE_MAX_FACES:
        raise ValueError(f"max_faces must lie in [1, {GATE_MAX_FACES}]")
    c = _gate_config(config)
    live_n = np.full(n, F, np.int64) if counts is None else np.clip(np.asarray(counts, np.int64).reshape(n), 0, F)
    live = np.arange(F)[None, :] < live_n[:, None]
    with np.errstate(all="ignore"):
        bbox = d[..., :4].astype(np.int32)
        score = d[..., 4].astype(np.float64)
        size = np.minimum(bbox[..., 2] - bbox[..., 0], bbox[..., 3] - bbox[..., 1])
        f32 = np.float32
        lex, ley, rex, rey, nx, ny, lmy, rmy = (d[..., k] for k in (5, 6, 7, 8, 9, 10, 12, 14))
        ecx, ecy = (lex + rex) / f32(2), (ley + rey) / f32(2)
        dx, dy = rex - lex, rey - ley
        dist = np.sqrt(dx * dx + dy * dy)
        ratio = (nx - ecx) / dist
        ratio = np.where(ratio < -1, f32(-1), np.where(ratio > 1, f32(1), ratio)).astype(f32)  # a NaN stays
        K = f32(180) / f32(np.pi)
        roll = np.arctan2(dy.astype(np.float64), dx.astype(np.float64)).astype(f32) * K
        yaw = np.arcsin(ratio.astype(np.float64)).astype(f32) * K * f32(2)
        pitch = ((ny - ecy) / ((lmy + rmy) / f32(2) - ecy) - f32(0.5)) * f32(60)
        assert roll.dtype == yaw.dtype == pitch.dtype == f32
        fail_score = score < c["min_det_score"]
        fail_size = size.astype(np.float64) < c["min_face_size"]
        fail_pose = ((np.abs(yaw) > f32(c["max_yaw"])) | (np.abs(pitch) > f32(c["max_pitch"]))
                     | (np.abs(roll) > f32(c["max_roll"])))
        check_blur = c["check_blur"] and blur is not None
        b = np.asarray(blur, np.float64).reshape(n, F) if check_blur else np.zeros((n, F))
        fail_blur = (b < c["blur_threshold"]) if check_blur else np.zeros((n, F), bool)
        fit = np.ones((n, F), bool) if ok is None else np.asarray(ok).reshape(n, F) != 0
    stage = np.select([~live, fail_score, fail_size, fail_pose, fail_blur, ~fit],
                      [GATE_NOT_LIVE, GATE_DET_SCORE, GATE_FACE_SIZE, GATE_POSE, GATE_BLUR, GATE_FIT],
                      GATE_VALID).astype(np.uint8)
    posed = live & ~fail_score & ~fail_size          # the pose angles were computed
    blurred = posed & ~fail_pose & check_blur        # the blur score was recorded
    metrics = np.zeros((n, F, 5))
    metrics[..., 0] = np.where(live, score, 0.0)
    metrics[..., 1] = np.where(blurred, b, 0.0)
    for k, a in ((2, yaw), (3, pitch), (4, roll)):
        metrics[..., k] = np.where(posed, a.astype(np.float64), 0.0)
    bbox = np.where(live[..., None], bbox, 0).astype(np.int32)
    with np.errstate(all="ignore"):
        key = score * np.where(blurred, b, 1000.0)
    rank = np.full((n, F), -1, np.int32)
    rows = np.full(n * F, -1, np.int32)
    valid_slots = np.full(n * F, -1, np.int32)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(live_n)
    for f in range(n):
        m = int(live_n[f])
        order = np.argsort(-key[f, :m], kind="stable")  # descending, equal keys by ascending slot
        rank[f, order] = np.arange(m, dtype=np.int32)
        rows[offsets[f]:offsets[f] + m] = f * F + order
    packed = rows[:offsets[n]]
    good = packed[stage.reshape(-1)[packed] == GATE_VALID]
    valid_slots[:good.size] = good
    return stage, metrics, bbox, rank, rows, offsets, valid_slots, np.array([good.size], np.int32)


def tensors_to_host(tensors: Dict[str, torch.Tensor]) -> Dict[str, np.ndarray]:
    """Device tensors -> host arrays of the same shapes and types in ONE copy (and one
    synchronisation): their bytes are concatenated on the device, widest element type first."""
    items = sorted(tensors.items(), key=lambda kv: -kv[1].element_size())
    parts = [t.contiguous().view(-1).view(torch.uint8) for _k, t in items]
    host = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, np.uint8)
    out, at = {}, 0
    for (k, t), p in zip(items, parts):
        out[k] = host[at:at + p.numel()].view(torch.empty(0, dtype=t.dtype).numpy().dtype).reshape(tuple(t.shape))
        at += p.numel()
    return out


def device_chain(detector, aligner, quality_filter, frames: torch.Tensor, max_faces: Optional[int] = None,
                 with_dets: bool = True):
    """Frames in HBM to gated, ranked faces in HBM: detect_device -> align_device ->
    blur_scores_device -> gate_device back to back with ``max_faces`` slots per frame (default: the
    detector's), then ONE copy of the per-slot outputs.  frames: uint8 [n,H,W,3] on the device ->
    ``(host, gate, crops)``: ``host`` the gate's outputs, ``counts`` and (``with_dets``) ``dets`` as
    host arrays, ``gate`` the gate's device tensors, ``crops`` uint8 [n*F,S,S,3] on the device, one
    per slot (all-zero where the slot is not live or its fit was refused).  Needs the GPU
    ``FaceDetector``: a detector without ``detect_device`` raises TypeError.  A frame over the
    detector's 4096-candidate limit raises the ``NotImplementedError`` ``FaceDetector.detect`` raises."""
    model = getattr(detector, "model", None)
    if not hasattr(model, "detect_device"):
        raise TypeError("the device chain runs the GPU FaceDetector (detect_device); this detector has none")
    n = frames.shape[0]
    F = detector.max_faces if max_faces is None else int(max_faces)
    S = aligner.output_size
    dets, counts = model.detect_device(frames, detector.det_thresh, F)
    crops, _, ok = aligner._ops.handle.align_device(frames, dets, counts, S)
    crops = crops.view(n * F, S, S, 3)
    blur = quality_filter._ops.handle.blur_scores_device(crops) if quality_filter.check_blur else None
    gate = quality_filter.gate_device(dets, counts, ok, blur)
    host = tensors_to_host({**gate, "counts": counts, **({"dets": dets} if with_dets else {})})
    for f in np.flatnonzero(host["counts"] < 0):
        raise NotImplementedError(f"frame {f} has more than 4096 anchors above det_thresh (limit 4096)")
    return host, gate, crops


def device_chain_images(detector, aligner, quality_filter, images, max_faces: Optional[int] = None,
                        with_dets: bool = True, pick=None):
    """``device_chain`` for a sequence of images of different sizes (host arrays or device tensors,
    RGB [H,W,3] or gray [H,W]): detect_images_device -> align_images_device -> blur_scores_device ->
    gate_device back to back, nothing staged and nothing waited for in between, in blocks of the
    detector's ``max_frames`` images with ONE packed copy of the per-slot outputs per block.  Returns
    what ``device_chain`` returns, ``(host, gate, crops)``, for the whole sequence: slot numbers
    (``rows`` / ``valid_slots``) count i * F + k over all images and ``frame_offsets`` runs over all of
    them, so ``chain_faces(quality_filter, host, i)`` lists image i.

    The crops of a block's slots take len(block) * F * S * S * 3 bytes.  With ``pick`` that is all
    the chain holds: ``pick(host, gate, crops)`` is called per block with the block's own outputs
    (slot numbers local to the block) and returns the crops to keep, a uint8 [m,S,S,3] device tensor
    (``crops[gate["rows"][:total].long()]``, say); the returned ``crops`` are the kept ones, block after
    block.  Without it the crops of every slot of every image are returned, [n*F,S,S,3].

    Needs the GPU ``FaceDetector``: a detector without ``detect_images_device`` raises TypeError.  An
    image over the detector's 4096-candidate limit raises the ``NotImplementedError``
    ``FaceDetector.detect_images`` raises."""
    model = getattr(detector, "model", None)
    if not hasattr(model, "detect_images_device"):
        raise TypeError("the device chain for images runs the GPU FaceDetector (detect_images_device); "
                        "this detector has none")
    dev = aligner._ops.device
    frames = [_device_frame(im, dev) for im in images]
    n = len(frames)
    F = detector.max_faces if max_faces is None else int(max_faces)
    S = aligner.output_size
    B = max(1, int(model.max_batch))
    hosts, gates, kept = [], [], []
    for first in range(0, max(n, 1), B):
        block = frames[first:first + B]
        dets, counts = model.detect_images_device(block, detector.det_thresh, F)
        crops, _, ok = aligner._ops.handle.align_images_device(block, dets, counts, S)
        crops = crops.view(len(block) * F, S, S, 3)
        blur = quality_filter._ops.handle.blur_scores_device(crops) if quality_filter.check_blur else None
        gate = quality_filter.gate_device(dets, counts, ok, blur)
        host = tensors_to_host({**gate, "counts": counts, **({"dets": dets} if with_dets else {})})
        for f in np.flatnonzero(host["counts"] < 0):
            raise NotImplementedError(f"image {first + f} has more than 4096 anchors above det_thresh (limit 4096)")
        hosts.append(host)
        gates.append(gate)
        kept.append(crops if pick is None else pick(host, gate, crops))
    if len(hosts) == 1:
        return hosts[0], gates[0], kept[0]
    return _merge_chain_blocks(hosts, F), _merge_chain_blocks(gates, F, hosts), torch.cat(kept)


def _merge_chain_blocks(blocks: List[Dict], F: int, hosts: Optional[List[Dict]] = None) -> Dict:
    """The gate outputs of consecutive blocks of images as those of one call over all of them: per-slot
    arrays back to back, the packed lists with each block's slot numbers moved behind the blocks before
    it.  ``blocks`` are host arrays, or (``hosts``: the same blocks on the host, for the totals)
    device tensors."""
    on_host = hosts is None
    hosts = blocks if on_host else hosts
    cat = np.concatenate if on_host else torch.cat
    out = {k: cat([b[k] for b in blocks]) for k in blocks[0] if k not in ("rows", "valid_slots", "frame_offsets",
                                                                           "n_valid")}
    rows, valid, offsets, first, faces = [], [], [blocks[0]["frame_offsets"][:1]], 0, 0
    for b, h in zip(blocks, hosts):
        nb = h["stage"].shape[0]
        rows.append(b["rows"][:int(h["frame_offsets"][nb])] + first * F)
        valid.append(b["valid_slots"][:int(h["n_valid"][0])] + first * F)
        offsets.append(b["frame_offsets"][1:] + faces)
        first += nb
        faces += int(h["frame_offsets"][nb])
    fill = (lambda m: np.full(m, -1, np.int32)) if on_host else (
        lambda m: torch.full((m,), -1, dtype=torch.int32, device=blocks[0]["rows"].device))
    n_valid = sum(int(h["n_valid"][0]) for h in hosts)
    out["rows"] = cat(rows + [fill(first * F - faces)])
    out["valid_slots"] = cat(valid + [fill(first * F - n_valid)])
    out["frame_offsets"] = cat(offsets)
    out["n_valid"] = blocks[0]["n_valid"] * 0 + n_valid
    return out


def chain_faces(quality_filter, host: Dict[str, np.ndarray], f: int) -> List[Dict]:
    """Frame ``f`` of ``device_chain``'s host outputs as ``process_numpy(frame, return_all=True)``
    lists it (descending det_score x blur_score, equal keys in detection order), each dict with
    ``'slot'`` (the index of its crop) in place of ``'aligned_face'``."""
    F = host["stage"].shape[1]
    out = []
    for slot in host["rows"][host["frame_offsets"][f]:host["frame_offsets"][f + 1]]:
        i = int(slot) - f * F
        stage = host["stage"][f, i]
        q = quality_filter.metrics_from_gate(stage, host["metrics"][f, i], host["bbox"][f, i])
        out.append({"slot": int(slot), "bbox": host["bbox"][f, i].copy(),
                    "landmarks": host["dets"][f, i, 5:15].reshape(5, 2).copy(), "det_score": q["det_score"],
                    "quality_metrics": q, "is_valid": bool(stage == GATE_VALID)})
    return out


def load_image_rgb(path: str) -> Optional[np.ndarray]:
    """cv2.cvtColor(cv2.imread(path), COLOR_BGR2RGB) through PIL: uint8 [H,W,3] RGB, or None when
    the file is missing or not a decodable image (cv2.imread returns None there).  imread's
    default IMREAD_COLOR makes every image 3-channel: gray and palette images are expanded, an
    alpha channel is dropped.  (8-bit images; imread's 16-bit down-conversion is not restated.)"""
    try:
        from PIL import Image
        with Image.open(path) as im:
            im.load()
            return np.array(im.convert("RGB"), dtype=np.uint8)  # a writable copy
    except (OSError, ValueError, SyntaxError):
        return None


class FaceDetector:
    """``FaceDetector`` (face_recognition.py:19-48) on the GPU: SCRFD-10G at ``det_size``,
    ``det_thresh``, NMS IoU 0.4; ``providers`` is accepted for signature parity."""

    def __init__(self, det_size=(640, 640), det_thresh=0.5, providers=None, model_path: Optional[str] = None,
                 state_dict=None, device=None, max_frames: int = 16, max_faces: int = 256):
        from .detector_arch import synthetic_detector_state_dict
        if tuple(det_size) != (640, 640):
            raise NotImplementedError("the MI355X detector is built for det_size=(640, 640) (the reference's setting)")
        self.det_size = tuple(det_size)
        self.det_thresh = float(det_thresh)
        self.max_faces = int(max_faces)
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        if state_dict is None:
            if model_path is not None:
                sd = torch.load(model_path, map_location="cpu", weights_only=True)
                state_dict = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
            else:
                state_dict = synthetic_detector_state_dict()
        self.model = _lib.Handle("scrfd_10g", "scrfd", self.device, max_batch=max_frames)
        self.model.load_state_dict({k: v for k, v in state_dict.items()})

    @staticmethod
    def _to_rgb(image: np.ndarray) -> np.ndarray:
        if image.ndim == 2:  # cv2.COLOR_GRAY2BGR replicates the channel (face_recognition.py:32-33)
            image = np.repeat(image[:, :, None], 3, axis=2)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"expected an HxW or HxWx3 image, got {image.shape}")
        return np.ascontiguousarray(image, dtype=np.uint8)

    @staticmethod
    def _faces(dets: np.ndarray, count: int) -> List[Dict]:
        out = []
        for i in range(count):
            d = dets[i]
            out.append({"bbox": d[:4].astype(np.int32), "landmarks": d[5:15].reshape(5, 2).astype(np.float32),
                        "det_score": float(d[4]), "pose": None, "age": None, "gender": None})
        return out

    def detect(self, image: np.ndarray) -> List[Dict]:
        """RGB (or gray) uint8 image -> [{'bbox' int32 x1y1x2y2, 'landmarks' f32 (5,2), 'det_score', ...}]
        in descending score order, like face_recognition.py:31-48."""
        frame = torch.from_numpy(self._to_rgb(image)).to(self.device)
        return self.detect_batch(frame[None])[0]

    def detect_batch(self, frames: torch.Tensor) -> List[List[Dict]]:
        """Device form: uint8 [n,H,W,3] RGB frames (one size) -> per-frame face lists."""
        dets, counts = self.model.detect(frames, self.det_thresh, self.max_faces)
        return [self._faces(dets[f], min(int(counts[f]), self.max_faces)) for f in range(dets.shape[0])]

    def detect_images(self, images) -> List[List[Dict]]:
        """``detect`` for a sequence of images of different sizes (host arrays or device tensors, RGB
        [H,W,3] or gray [H,W]) in one call -> per-image face lists.  The images run in input order in
        chunks of ``max_frames``, each with its own letterbox geometry (``fr_detect_images``)."""
        frames = [_device_frame(im, self.device) for im in images]
        dets, counts = self.model.detect_images(frames, self.det_thresh, self.max_faces)
        return [self._faces(dets[f], min(int(counts[f]), self.max_faces)) for f in range(len(frames))]


class FaceProcessor:
    """detect -> align -> quality (face_recognition.py:160-216) with device alignment and blur."""

    def __init__(self, output_size=224, det_size=(640, 640), det_thresh=0.5,
                 quality_filter_config: Optional[Dict] = None, providers=None, detector=None, device=None):
        self.detector = detector if detector is not None else FaceDetector(det_size, det_thresh, providers,
                                                                           device=device)
        self.aligner = FaceAligner(output_size=output_size, device=device)
        self.quality_filter = FaceQualityFilter(**(quality_filter_config or {}), device=device)

    def process_image(self, image_path: str, return_all: bool = False) -> List[Dict]:
        """face_recognition.py:174-182: read the file, convert to RGB, process_numpy.  The file is
        decoded by PIL (cv2 is not in the image): lossless formats (PNG, BMP, TIFF) decode to the
        same bytes cv2.imread gives; JPEG decoders may differ in rounding, so JPEG parity with
        cv2.imread is unpinned.  Like cv2.imread, a file that cannot be read raises ValueError."""
        image_rgb = load_image_rgb(image_path)
        if image_rgb is None:
            raise ValueError(f"Could not load image: {image_path}")
        return self.process_numpy(image_rgb, return_all)

    def process_images(self, images, return_all: bool = False, errors: str = "raise", gate: str = "host") -> List:
        """``process_numpy`` / ``process_image`` for a sequence of images of different sizes -- arrays
        (RGB [H,W,3] or gray [H,W]) or paths, mixed freely -- with the GPU work batched across the
        sequence: one ``detect_images`` call (chunked by the detector's ``max_frames``), one
        ``align_images`` launch over all faces of all images, one blur call over all crops.  Returns one
        result list per item, each what ``process_numpy`` returns for that image (the same gate, sort
        and dicts).  A detector without ``detect_images`` (a user-supplied ``detector=``) is asked
        ``detect`` per image; alignment and blur are batched all the same.

        An item that cannot be used -- a path that does not decode (``process_image``'s ValueError),
        an array that is no HxW / HxWx3 image -- is reported as ``errors`` says: "raise" (default)
        raises its ValueError before any GPU work, so nothing is half done; "return" puts the
        ValueError instance in that item's slot of the returned list and processes the other items, so
        one bad file does not lose the batch (``DatasetPreprocessor``).  JPEG parity as in
        ``process_image``.

        Against ``process_numpy`` per image: with a detector of fixed answers the results are equal bit
        for bit.  With the GPU detector an image runs the same network in another batch, so its head
        maps differ by fp32 rounding: the same faces, det_score within 1e-5 and boxes within 1 px where
        scores are distinct.  On smooth content (a wall, a sky, a tiny image upscaled) neighbouring
        anchors score equal to the last bits, and NMS may then keep a neighbouring box of the same
        score in one path and not the other ("Mixed-size image batches").

        ``gate="device"`` keeps the whole pass on the device (``device_chain_images``): detections are
        fitted, warped, scored and gated where they are, one packed copy per block of the detector's
        ``max_frames`` images brings the per-slot outputs over, and only the crops that are returned --
        every live one (``return_all``) or the first valid one of each image -- are gathered on the
        device (through the gate's ``rows`` / ``valid_slots``) and copied.  Against ``gate="host"``:
        the same faces in the same order, the same ``is_valid``, boxes, landmarks and crop bytes;
        metrics as ``process_frames`` states.  A detection whose similarity fit fails comes back
        ``is_valid: False`` with an all-zero crop, where the host path raises.  Needs the GPU
        ``FaceDetector`` (TypeError otherwise)."""
        if gate not in ("host", "device"):
            raise ValueError('gate must be "host" or "device"')
        if gate == "device":
            return self._process_images_device(images, return_all, errors)
        out, items, faces, crops, blur = self._detect_align_images(images, errors)
        at = 0
        for (slot, image), fs in zip(items, faces):
            # to the host image by image: a block per image, as process_numpy's, not one block for the
            # whole call (hundreds of MB for a chunk of group photographs, freshly paged in every call)
            mine = crops[at:at + len(fs)].cpu().numpy()
            if image.ndim == 2:  # a gray image's crops go back 2-D, as in process_numpy
                mine = np.ascontiguousarray(mine[..., 0])
            out[slot] = self._gate(fs, mine, None if blur is None else blur[at:at + len(fs)], return_all) if fs else []
            at += len(fs)
        return out

    def _detect_align_images(self, images, errors: str):
        """The GPU pass of ``process_images``: -> (out, items, faces, crops, blur).  ``out`` has one slot
        per item of ``images``, None or the ValueError of an item that cannot be used; ``items`` the
        usable ones as (slot, image as process_numpy would get it); ``faces[j]`` the detector's faces of
        ``items[j]``; ``crops`` uint8 [total,S,S,3] on the device, image by image in face order; ``blur``
        their float64 blur scores on the host, or None (not checked, or no face)."""
        out, items = self._usable_items(images, errors)
        dev = self.aligner._ops.device
        frames = [_device_frame(image, dev) for _slot, image in items]
        if hasattr(self.detector, "detect_images"):
            faces = self.detector.detect_images(frames) if frames else []
        else:
            faces = [self.detector.detect(image) for _slot, image in items]
        crops = self.aligner.align_images(frames, [np.stack([f["landmarks"] for f in fs]) if fs else
                                                   np.zeros((0, 5, 2), np.float32) for fs in faces])
        blur = (self.quality_filter.compute_blur_scores(crops)
                if self.quality_filter.check_blur and crops.shape[0] else None)
        return out, items, faces, crops, blur

    @staticmethod
    def _usable_items(images, errors: str):
        """-> (out, items): ``out`` one slot per item of ``images``, None or the ValueError of an item that
        cannot be used; ``items`` the usable ones as (slot, image as process_numpy would get it)."""
        if errors not in ("raise", "return"):
            raise ValueError('errors must be "raise" or "return"')
        out: List = [None] * len(images)
        items = []  # (slot, the image as process_numpy would get it)
        for slot, item in enumerate(images):
            try:
                if isinstance(item, (str, bytes)) or hasattr(item, "__fspath__"):
                    image = load_image_rgb(item)
                    if image is None:
                        raise ValueError(f"Could not load image: {item}")
                else:
                    image = np.asarray(item)
                    FaceDetector._to_rgb(image)  # the shape check of detect
            except ValueError as e:
                if errors == "raise":
                    raise
                out[slot] = e
                continue
            items.append((slot, image))
        return out, items

    def _chain_images(self, images, return_all: bool):
        """``device_chain_images`` over usable images, keeping on the device only the crops a caller
        hands on -- every live one in result order (``return_all``) or the first valid one of each
        image -- -> (per_image, crops): ``per_image[j]`` image j's ``chain_faces`` dicts that are kept,
        ``crops`` uint8 [m,S,S,3] on the device, one per kept face, image after image."""
        model = getattr(self.detector, "model", None)
        if not hasattr(model, "detect_images_device"):
            raise TypeError("the device chain for images runs the GPU FaceDetector (detect_images_device); "
                            "this detector has none")
        F = self.detector.max_faces

        def pick(host, gate, crops):
            if return_all:
                picked = gate["rows"][:int(host["frame_offsets"][-1])]  # the live slots, image by image
            else:
                valid = host["valid_slots"][:int(host["n_valid"][0])]
                first = np.flatnonzero(np.diff(valid // F, prepend=-1) != 0)  # the first valid slot of each image
                picked = gate["valid_slots"][torch.from_numpy(first).to(crops.device)]
            return crops[picked.long()]

        host, _gate, crops = device_chain_images(self.detector, self.aligner, self.quality_filter, images, F,
                                                 pick=pick)
        per_image = [chain_faces(self.quality_filter, host, j) for j in range(len(images))]
        if not return_all:
            per_image = [[x for x in faces if x["is_valid"]][:1] for faces in per_image]
        return per_image, crops

    def _process_images_device(self, images, return_all: bool, errors: str) -> List:
        if not hasattr(getattr(self.detector, "model", None), "detect_images_device"):
            raise TypeError("gate=\"device\" runs the GPU FaceDetector (detect_images_device); this detector has none")
        out, items = self._usable_items(images, errors)
        if not items:
            return out
        per_image, crops = self._chain_images([image for _slot, image in items], return_all)
        aligned = crops.cpu().numpy()
        at = 0
        for (slot, image), faces in zip(items, per_image):
            res = []
            for x in faces:
                crop = aligned[at]
                at += 1
                if image.ndim == 2:  # a gray image's crops go back 2-D, as in process_numpy
                    crop = np.ascontiguousarray(crop[..., 0])
                res.append({"aligned_face": crop, **{k: x[k] for k in ("bbox", "landmarks", "det_score",
                                                                        "quality_metrics", "is_valid")}})
            out[slot] = res
        assert at == len(aligned)
        return out

    def process_numpy(self, image_rgb: np.ndarray, return_all: bool = False) -> List[Dict]:
        faces = self.detector.detect(image_rgb)
        if len(faces) == 0:
            return []
        # a grayscale frame is warped as three equal channels: each channel of the warp is the
        # reference's single-channel warpAffine (face_recognition.py:72-74), and RGB2GRAY of
        # (g, g, g) is g, so the blur score is the reference's on the 2-D crop (:94-99); the
        # aligned face is handed back 2-D, as the reference's is
        gray = np.ndim(image_rgb) == 2
        frame = torch.from_numpy(FaceDetector._to_rgb(image_rgb)).to(self.aligner._ops.device)
        crops = self.aligner.align_batch(frame, np.stack([f["landmarks"] for f in faces]))
        blur = self.quality_filter.compute_blur_scores(crops) if self.quality_filter.check_blur else None
        host = crops.cpu().numpy()
        if gray:
            host = np.ascontiguousarray(host[..., 0])
        return self._gate(faces, host, blur, return_all)

    def process_frames(self, frames, return_all: bool = False, max_faces: Optional[int] = None) -> List[List[Dict]]:
        """``process_numpy`` for a batch of uint8 [n,H,W,3] RGB frames of one size (host array or
        device tensor) with the whole chain on the device -> one list per frame of ``process_numpy``'s
        dicts: detect_device -> align_device -> blur_scores_device -> gate_device run back to back
        (``device_chain``), ONE packed copy brings the per-slot outputs over, and the crops that are
        returned -- every live one (``return_all``) or the first valid one of each frame -- are gathered
        on the device through the gate's ``rows`` / ``valid_slots`` before they are copied.  Crops of
        every slot are held meanwhile: n * max_faces * S * S * 3 bytes (``max_faces`` defaults to the
        detector's).

        Against ``process_numpy`` per frame: the same faces in the same order, the same ``is_valid``
        and crop bytes; metrics as ``quality_gate_host`` states (yaw and roll within 1e-4 degrees of
        numpy's, all else bitwise).  A frame over the detector's 4096-candidate limit raises the
        ``NotImplementedError`` ``FaceDetector.detect`` raises for it; a detection whose similarity fit
        fails (where ``process_numpy`` raises) comes back ``is_valid: False`` with an all-zero crop."""
        dev = self.aligner._ops.device
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8))
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("expected uint8 [n,H,W,3] RGB frames")
        n = t.shape[0]
        if n == 0:
            return []
        host, gate, crops = device_chain(self.detector, self.aligner, self.quality_filter, t.to(dev).contiguous(),
                                         max_faces)
        F = host["stage"].shape[1]
        per_frame = [chain_faces(self.quality_filter, host, f) for f in range(n)]
        if return_all:
            total = int(host["frame_offsets"][n])
            picked = gate["rows"][:total]  # the live slots, frame by frame in result order
        else:
            valid = host["valid_slots"][:int(host["n_valid"][0])]
            first = np.flatnonzero(np.diff(valid // F, prepend=-1) != 0)  # the first valid slot of each frame
            picked = gate["valid_slots"][torch.from_numpy(first).to(dev)]
            keep = set(valid[first].tolist())
            per_frame = [[x for x in faces if x["slot"] in keep] for faces in per_frame]
        aligned = crops[picked.long()].cpu().numpy()
        at = 0
        for faces in per_frame:
            for x in faces:
                del x["slot"]
                x["aligned_face"] = aligned[at]
                at += 1
        assert at == len(aligned)
        return [[{k: x[k] for k in ("aligned_face", "bbox", "landmarks", "det_score", "quality_metrics", "is_valid")}
                 for x in faces] for faces in per_frame]

    def _gate(self, faces: List[Dict], host: np.ndarray, blur, return_all: bool) -> List[Dict]:
        """The host gate, sort and result dicts of one image (face_recognition.py:192-216): ``host[i]``
        the aligned crop and ``blur[i]`` the blur score (``blur`` None: not checked) of ``faces[i]``."""
        results = []
        for i, face in enumerate(faces):
            ok, q = self.quality_filter.is_valid(face, None, None if blur is None else float(blur[i]))
            if ok or return_all:
                results.append({"aligned_face": host[i], "bbox": face["bbox"], "landmarks": face["landmarks"],
                                "det_score": face["det_score"], "quality_metrics": q, "is_valid": ok})
        results.sort(key=lambda x: x["det_score"] * x["quality_metrics"].get("blur_score", 1000), reverse=True)
        if not return_all and results:
            return [results[0]]
        return results
