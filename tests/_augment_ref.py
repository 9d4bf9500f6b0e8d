"""numpy restatement of the reference's ``augment_face_for_enrollment`` (enroll_students.py:20-48)
for its first 14 list entries: what ``fr_augment_faces`` is pinned to, bit for bit.

Flip, brightness and contrast are the reference's own numpy expressions (``cv2.flip(img, 1)`` is
``img[:, ::-1]``).  The rotation restates ``cv2.getRotationMatrix2D`` + ``cv2.warpAffine(...,
INTER_LINEAR, BORDER_REPLICATE)`` with the fixed-point arithmetic of ``oracle.align_ref``
(``invert_affine`` and the ``warp_maps`` map, here for a W x H output) and OpenCV's
remapBilinear replicate branch: each of the four taps is clamped to the image on its own.
PARITY with cv2 itself is UNPINNED (cv2 is absent), as for the alignment warp.
"""
import math

import numpy as np

from oracle import align_ref as A

ANGLES = (-10, -5, 5, 10)
BETAS = (-20, -10, 10, 20)
ALPHAS = (0.85, 0.92, 1.08, 1.15)
MAX_VARIANTS = 14


def rotation_matrix(center, angle, scale=1.0) -> np.ndarray:
    """cv2.getRotationMatrix2D (imgwarp.cpp), double; math.cos / math.sin are libm's, as std::cos."""
    rad = angle * (math.pi / 180)
    a, b = math.cos(rad) * scale, math.sin(rad) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)


def warp_maps_wh(M_fwd: np.ndarray, W: int, H: int):
    """``oracle.align_ref.warp_maps`` for a W x H output."""
    Mi = A.invert_affine(M_fwd)
    xs, ys = np.arange(W), np.arange(H)
    adelta = A._cvround(Mi[0, 0] * xs * A.AB_SCALE)
    bdelta = A._cvround(Mi[1, 0] * xs * A.AB_SCALE)
    X0 = A._cvround((Mi[0, 1] * ys + Mi[0, 2]) * A.AB_SCALE) + A.ROUND_DELTA
    Y0 = A._cvround((Mi[1, 1] * ys + Mi[1, 2]) * A.AB_SCALE) + A.ROUND_DELTA
    X = (X0[:, None] + adelta[None, :]) >> (A.AB_BITS - A.INTER_BITS)
    Y = (Y0[:, None] + bdelta[None, :]) >> (A.AB_BITS - A.INTER_BITS)
    return X, Y


def warp_affine_replicate(img: np.ndarray, M_fwd: np.ndarray) -> np.ndarray:
    """cv2.warpAffine(img, M, (W, H), INTER_LINEAR, borderMode=BORDER_REPLICATE), uint8 HxWxC."""
    H, W = img.shape[:2]
    X, Y = warp_maps_wh(M_fwd, W, H)
    sx, fx = X >> A.INTER_BITS, X & (A.INTER_TAB - 1)
    sy, fy = Y >> A.INTER_BITS, Y & (A.INTER_TAB - 1)
    w00 = (A.INTER_TAB - fx) * (A.INTER_TAB - fy) * 32
    w01 = fx * (A.INTER_TAB - fy) * 32
    w10 = (A.INTER_TAB - fx) * fy * 32
    w11 = fx * fy * 32
    src = img.astype(np.int64)
    x0, x1 = np.clip(sx, 0, W - 1), np.clip(sx + 1, 0, W - 1)
    y0, y1 = np.clip(sy, 0, H - 1), np.clip(sy + 1, 0, H - 1)
    acc = (src[y0, x0] * w00[..., None] + src[y0, x1] * w01[..., None] +
           src[y1, x0] * w10[..., None] + src[y1, x1] * w11[..., None])
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def rotate(img: np.ndarray, angle) -> np.ndarray:
    center = (img.shape[1] // 2, img.shape[0] // 2)
    return warp_affine_replicate(img, rotation_matrix(center, angle, 1.0))


def flip(img: np.ndarray) -> np.ndarray:
    return img[:, ::-1].copy()


def brightness(img: np.ndarray, beta) -> np.ndarray:
    return np.clip(img.astype(np.float32) + beta, 0, 255).astype(np.uint8)


def contrast(img: np.ndarray, alpha) -> np.ndarray:
    return np.clip(img.astype(np.float32) * alpha, 0, 255).astype(np.uint8)


def augment(img: np.ndarray, num_augmentations: int = 8):
    """The reference's list, cut to ``num_augmentations`` <= 14."""
    assert num_augmentations <= MAX_VARIANTS
    out = [img.copy(), flip(img)]
    out += [rotate(img, a) for a in ANGLES]
    out += [brightness(img, b) for b in BETAS]
    out += [contrast(img, a) for a in ALPHAS]
    return out[:num_augmentations]


def augment_batch(crops: np.ndarray, num_augmentations: int) -> np.ndarray:
    """uint8 [n,H,W,3] -> [n,A,H,W,3]."""
    n, H, W, C = crops.shape
    out = np.empty((n, num_augmentations, H, W, C), np.uint8)
    for i in range(n):
        for v, a in enumerate(augment(crops[i], num_augmentations)):
            out[i, v] = a
    return out
