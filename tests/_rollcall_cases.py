"""Shared by test_photo_rollcall.py / test_gpu_photo_rollcall.py: seeded top-k-shaped inputs of
``fr_photo_rollcall`` (idx int32 / score float32 [total,k], CSR offsets) and two independent statements
of its rule.  Scores descend along a face's columns (NaNs aside), rows are distinct within a face, and
some rows are near 2e9: a kernel that used a row as an index would leave its buffers there.
"""
from __future__ import annotations

import numpy as np

RECOGNIZED, CANDIDATE, DISPLACED = 0, 1, 2
INDEPENDENT, EXCLUSIVE = 0, 1
THRESHOLDS = (0.35, 0.0, -0.2, float("inf"))
EDGE_COUNTS = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024)
# a grid straddling every finite threshold, both zeros included: exact ties across faces and columns
GRID = np.array([-0.4, -0.25, -0.2, -0.1, -0.0, 0.0, 0.1, 0.3, 0.34999999, 0.35, 0.36, 0.5, 0.7, 0.9],
                np.float32)


def _rows(r, pool):
    """``pool`` distinct row values: small ones, and a third of them near 2e9."""
    small = r.choice(100000, size=pool, replace=False).astype(np.int64)
    small[::3] += 2_000_000_000
    return small.astype(np.int32)


def random_case(seed, counts, k, pool):
    """Faces that draw ``k`` distinct rows from ``pool`` row values (a small pool: heavy contention)
    and grid scores sorted descending."""
    r = np.random.Generator(np.random.PCG64(seed))
    rows = _rows(r, max(pool, k))
    total = int(np.sum(counts))
    idx = np.stack([r.choice(rows, size=k, replace=False) for _ in range(total)]) if total else \
        np.zeros((0, k), np.int32)
    score = -np.sort(-GRID[r.integers(0, len(GRID), size=(total, k))], axis=1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return {"idx": idx.astype(np.int32), "score": score.astype(np.float32), "offsets": offsets}


def _one_photo(idx, score):
    idx, score = np.asarray(idx, np.int32), np.asarray(score, np.float32)
    return {"idx": idx, "score": score, "offsets": np.array([0, idx.shape[0]], np.int32)}


def planted_cases():
    out = {}
    # every face wants one row, k = 1: distinct scores, then all equal (the lowest face wins)
    n = 70
    out["one_row_k1"] = _one_photo(np.full((n, 1), 2_000_000_123), (0.4 + 0.005 * ((np.arange(n) * 37) % n))[:, None])
    out["one_row_k1_tied"] = _one_photo(np.full((n, 1), 7), np.full((n, 1), 0.5))
    # a displacement chain of length 50: face 0 takes row 1; face j wanted row j first and falls to
    # row j + 1, which face j + 1 wanted first, and so on; the third column is below every claim
    L = 50
    idx = np.zeros((L + 1, 3), np.int64)
    score = np.zeros((L + 1, 3), np.float64)
    idx[0], score[0] = (1, 1_999_999_000, 1_999_999_001), (0.99, 0.36, -0.3)
    for j in range(1, L + 1):
        idx[j] = (j, j + 1, 1_999_999_000 + 2 * j)
        score[j] = (0.99 - 0.01 * j + 0.004, 0.99 - 0.01 * j, -0.3)
    out["chain_50"] = _one_photo(idx, score)
    # exact ties across faces: the same score on the same first row, then on the second
    out["ties_across_faces"] = _one_photo([[5, 6, 7], [5, 6, 7], [5, 6, 7], [5, 6, 7], [8, 5, 6]],
                                          [[0.5, 0.5, 0.4], [0.5, 0.5, 0.4], [0.5, 0.45, 0.4], [0.5, 0.5, 0.5],
                                           [0.5, 0.5, 0.5]])
    # exact ties across columns: the lower column goes first
    out["ties_across_columns"] = _one_photo([[3, 4, 5], [4, 3, 5], [5, 4, 3], [2_000_000_001, 3, 4]],
                                            [[0.6, 0.6, 0.6], [0.6, 0.6, 0.1], [0.7, 0.7, 0.7], [0.0, -0.0, -0.0]])
    # NaN at column 0: never a claim, the columns behind it still are
    nan = float("nan")
    out["nan_column0"] = _one_photo([[9, 10, 11], [10, 9, 12], [13, 14, 15], [9, 13, 10]],
                                    [[nan, 0.8, 0.7], [0.9, 0.5, 0.4], [nan, nan, nan], [0.75, nan, 0.1]])
    # all scores below every finite threshold
    out["all_below"] = _one_photo([[1, 2], [1, 3], [2, 1]], [[-0.5, -0.6], [-0.3, -0.7], [-0.21, -0.9]])
    return out


def cases():
    """name -> {'idx', 'score', 'offsets'}."""
    out = planted_cases()
    out["edge_counts_contended"] = random_case(1, EDGE_COUNTS, 5, 40)
    out["edge_counts_spread"] = random_case(2, EDGE_COUNTS[::-1], 3, 3000)
    r = np.random.Generator(np.random.PCG64(3))
    for i, k in enumerate((1, 3, 5, 16)):
        out[f"images_300_k{k}"] = random_case(10 + i, r.integers(0, 13, size=300), k, 30)
        out[f"images_1_k{k}"] = random_case(20 + i, [40 + i], k, 25)
    out["no_faces"] = random_case(30, [0, 0, 0], 2, 4)
    return out


def independent_rule(idx, score, offsets, thr):
    """The reference's line: ``recognized = score >= self.similarity_threshold`` on the top-1."""
    status = np.array([RECOGNIZED if float(s) >= thr else CANDIDATE for s in score[:, 0]], np.int32)
    face = np.stack([status, idx[:, 0], np.zeros_like(status), np.zeros_like(status)], axis=1).astype(np.int32)
    image = np.array([[b - a, (status[a:b] == RECOGNIZED).sum(), (status[a:b] == CANDIDATE).sum(), 0]
                      for a, b in zip(offsets[:-1], offsets[1:])], np.int32).reshape(-1, 4)
    return face, score[:, 0].copy(), image


def exclusive_brute_force(idx, score, offsets, thr):
    """The exclusive rule by repeated global argmax: of the claims whose face is free and whose row is
    free, grant the one with the highest score (then the lowest face, then the lowest column), until
    none is left."""
    total, k = idx.shape
    face = np.zeros((total, 4), np.int32)
    out_score = np.zeros(total, np.float32)
    image = np.zeros((len(offsets) - 1, 4), np.int32)
    with np.errstate(invalid="ignore"):
        claim = score.astype(np.float64) >= thr
    for p, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        a, b = int(a), int(b)
        rows, sc, cl = idx[a:b], score[a:b], claim[a:b]
        free = np.ones(b - a, bool)
        held = np.zeros(0, np.int32)
        got = {}
        while True:
            open_ = cl & free[:, None] & ~np.isin(rows, held)
            cand = np.flatnonzero(open_.ravel())
            if cand.size == 0:
                break
            s = sc.ravel()[cand]
            best = int(cand[s == s.max()].min())  # flat index = face * k + column
            f, c = divmod(best, k)
            got[f] = c
            free[f] = False
            held = np.append(held, rows[f, c])
        for f in range(b - a):
            c = got.get(f, 0)
            status = RECOGNIZED if f in got else DISPLACED if cl[f, 0] else CANDIDATE
            face[a + f] = (status, rows[f, c], c, 0)
            out_score[a + f] = sc[f, c]
            image[p, 1 + status] += 1
        image[p, 0] = b - a
    return face, out_score, image


def same(got, want):
    """The three outputs equal bit for bit (the scores as bits: NaNs included)."""
    return (np.array_equal(np.asarray(got[0], np.int32), want[0])
            and np.asarray(got[1], np.float32).tobytes() == np.asarray(want[1], np.float32).tobytes()
            and np.array_equal(np.asarray(got[2], np.int32), want[2]))
