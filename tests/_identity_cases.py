"""Shared by test_match_identities.py and test_gpu_match_identities.py: the order rule a top-k over
identity scores is held to, and the seeded gallery of the tile / lane edge test.

The order rule.  The reference order of a probe is the stable descending order of its reference
scores (Python's ``sorted(..., reverse=True)`` over the dict order: equal scores keep the lower
identity index first).  Reference positions whose scores are less than ``EC.MARGIN`` apart are joined
into a group; a returned identity must sit in the group of the position it is returned at.  A
position at least MARGIN away from both neighbours is a group of its own, so it must hold exactly the
reference's identity; positions joined by smaller gaps may permute among themselves, and only there.
"""
import numpy as np

from tests import _eval_cases as EC

f32 = np.float32


def stable_order(scores):
    """Descending, equal scores in index order."""
    return np.argsort(-np.asarray(scores), axis=1, kind="stable")


def near_pairs(ref_scores, depth):
    """How many adjacent pairs (j, j + 1), j < depth, of the reference order are less than MARGIN apart."""
    ref = np.asarray(ref_scores, np.float64)
    srt = np.take_along_axis(ref, stable_order(ref), axis=1)
    gaps = srt[:, :-1] - srt[:, 1:]
    return int((gaps[:, :depth] < EC.MARGIN).sum())


def check_topk(idx, score, ref_scores, k, exact=False, tol=EC.SCORE_TOL):
    """``idx`` / ``score`` [n,k] against reference scores [n,n_ids] under the order rule; returns the
    number of excused positions (positions that hold another identity than the reference order's).
    ``exact``: the reference order and the reference's score bits, nothing excused."""
    ref = np.asarray(ref_scores, f32)
    n, n_ids = ref.shape
    idx, score = np.asarray(idx), np.asarray(score)
    assert idx.shape == (n, k) and score.shape == (n, k) and idx.dtype == np.int32 and score.dtype == f32
    order = stable_order(ref)
    if exact:
        assert np.array_equal(idx, order[:, :k])
        assert score.tobytes() == np.take_along_axis(ref, order[:, :k], axis=1).tobytes()
        return 0
    assert idx.min() >= 0 and idx.max() < n_ids
    assert all(len(set(r)) == k for r in idx.tolist()), "an identity returned twice"
    assert np.abs(score.astype(np.float64) - np.take_along_axis(ref, idx.astype(np.int64), axis=1)).max() <= tol
    assert np.all(score[:, :-1] >= score[:, 1:]), "scores must descend"
    srt = np.take_along_axis(ref, order, axis=1).astype(np.float64)
    group = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(srt[:, :-1] - srt[:, 1:] >= EC.MARGIN, axis=1)], axis=1)
    position = np.argsort(order, axis=1)  # identity -> its position in the reference order
    got_group = np.take_along_axis(group, np.take_along_axis(position, idx.astype(np.int64), axis=1), axis=1)
    assert np.array_equal(got_group, group[:, :k]), "an identity outside the group of its position"
    return int((idx != order[:, :k]).sum())


# ---------------------------------------------------------------------------------------------
# tile and lane edges
# ---------------------------------------------------------------------------------------------
# rows on both sides of every 4-lane / 64-row step and of the serving tile caps, identities of the
# kernels' longest length, and more than EVAL_TILE_IDS identities in a row for the composed path
EDGE_LENGTHS = [1, 1, 2, 3, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1, 5] + [1] * 1100 + [1024, 1024, 1, 7]
EDGE_SEED = 0x1DE7_0001
EDGE_QUERIES = 40
EDGE_RUNS = (("max", 3), ("mean", 3), ("topk", 1), ("topk", 3), ("topk", 16))


def edge_case(seed=EDGE_SEED):
    """(Q [40,512], E [G,512], offsets): unit rows around seeded centres as ``EC.seeded_case`` builds
    them; a query leans on two or three centres, so the best identities are well apart and the long
    tail of unrelated identities is not."""
    r = np.random.Generator(np.random.PCG64(seed))
    n_ids = len(EDGE_LENGTHS)
    cent = EC._unit(r.standard_normal((n_ids, 512)))
    E = np.concatenate([EC._unit(cent[i][None, :] + 0.02 * r.standard_normal((n, 512)))
                        for i, n in enumerate(EDGE_LENGTHS)])
    offsets = np.concatenate([[0], np.cumsum(EDGE_LENGTHS)]).astype(np.int32)
    Q = []
    for p in range(EDGE_QUERIES):
        ids = r.choice(n_ids, size=3, replace=False)
        if p % 4 == 0:
            ids[0] = (5, 8, 11, 12, 1115, 1116, 9, 6, 7, 10)[(p // 4) % 10]  # the long identities in turn
        w = np.array([0.8, 0.45, 0.3]) * (1 + 0.1 * r.standard_normal(3))
        Q.append(EC._unit(w @ cent[ids].astype(np.float64) + 0.012 * r.standard_normal(512)))
    return np.stack(Q).astype(f32), E.astype(f32), offsets
