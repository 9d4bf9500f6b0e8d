"""Landmark sets for the similarity-fit tests (tests/test_gpu_device_chain.py) and for
tools/fit_check.cpp: float32 [n, 5, 2] frame landmarks that fit_similarity maps to the reference
template of ``out_size``.  Deterministic; the first seven sets are the special cases, the rest the
template under random similarities with 0-6 px of noise in template space (the inlier bar is 3 px
there, so some sets have outliers and RANSAC runs several iterations).

``python tests/_fit_sets.py OUT_SIZE FILE`` writes the sets as raw float32 for tools/fit_check.cpp.
"""
import sys

import numpy as np

TEMPLATE = np.array([[0.34, 0.46], [0.66, 0.46], [0.50, 0.61], [0.37, 0.74], [0.63, 0.74]], dtype=np.float64)
N_SETS = 130


def template(out_size: int) -> np.ndarray:
    return (TEMPLATE * out_size).astype(np.float32)


def _similarity(rng, shift=1000.0):
    s = rng.uniform(0.3, 3.0)
    a = rng.uniform(-np.pi, np.pi)
    R = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return R, rng.uniform(0.0, shift, size=2)


def landmark_sets(out_size: int, n: int = N_SETS) -> np.ndarray:
    rng = np.random.default_rng(1000 + out_size)
    t = template(out_size).astype(np.float64)
    sets = []
    # the exact template: all inliers on the first model, the iteration count drops to 0
    sets.append(t.copy())
    # five equal points: every 2-point model is degenerate, the host fit fails
    sets.append(np.full((5, 2), 321.5))
    # two coincident points among five
    R, T = _similarity(rng)
    lm = t @ R.T + T
    lm[3] = lm[1]
    sets.append(lm)
    # exactly k planted inliers: the others sit 30-60 px away in template space
    for k in (2, 3, 4):
        R, T = _similarity(rng)
        q = t.copy()
        for j in range(k, 5):
            ang = rng.uniform(0, 2 * np.pi)
            q[j] += rng.uniform(30, 60) * np.array([np.cos(ang), np.sin(ang)])
        sets.append(q @ R.T + T)
    # coordinates around 1e4
    R, T = _similarity(rng)
    sets.append(t @ R.T + T + 1e4)
    while len(sets) < n:
        R, T = _similarity(rng, shift=1e4 if len(sets) % 9 == 0 else 1000.0)
        ang = rng.uniform(0, 2 * np.pi, size=5)
        mag = rng.uniform(0.0, 6.0, size=5)
        noise = mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        sets.append((t + noise) @ R.T + T)
    if n > 64:
        sets[64] = np.zeros((5, 2))  # a second set the host refuses, in the second block's first lane
    return np.ascontiguousarray(np.stack(sets[:n]), dtype=np.float32)


if __name__ == "__main__":
    landmark_sets(int(sys.argv[1])).tofile(sys.argv[2])
