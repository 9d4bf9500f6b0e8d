"""topk_small_kernel<8> and topk_kernel (embed_misc.hip) at their dispatch seam and on planted rows.

Both kernels, in both tie orders (frt_topk_ex: index descending, the gallery search's order, and
index ascending, fr_match_identities'), against a plain restatement of the rule: NaN never ranks,
the rest sorts by (score descending, then index), a row with fewer than k rankable scores ends in
idx -1 / val -inf.  idx and val are compared bit for bit (val is a copy of an input score, so -0.0
and 0.0 tell apart which of two equal scores was taken), and every launch runs twice and must
return the same bits.

launch_topk_order takes topk_small_kernel<8> (one block per row, 8 candidates per thread) for
k <= 8 and topk_kernel (one wave per row, 4 rows per block) above; the small kernel reads float4
when G % 4 == 0 and the row is 16-byte aligned, scalars otherwise.  The shapes here sit on each of
those conditions' two sides.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _frt

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF, NAN = np.float32(np.inf), np.float32(np.nan)
ORDERS = pytest.mark.parametrize("low_first", [False, True], ids=["high_first", "low_first"])


def ref_topk(s, k, low_first):
    """The rule restated: per row drop NaN, sort by (score desc, index asc with low_first, else index
    desc), pad with idx -1 / val -inf.  (oracle.reference_path.topk_policy is the high-index-first
    rule for NaN-free rows with k <= G rankable entries: its lexsort would rank a NaN.)"""
    n, G = s.shape
    idx = np.full((n, k), -1, dtype=np.int32)
    val = np.full((n, k), -np.inf, dtype=np.float32)
    for r in range(n):
        cols = [g for g in range(G) if not np.isnan(s[r, g])]
        cols.sort(key=lambda g: (-float(s[r, g]), g if low_first else -g))
        cols = cols[:k]
        idx[r, :len(cols)] = cols
        val[r, :len(cols)] = s[r, cols]
    return idx, val


def _frozen(a):
    a.setflags(write=False)  # shared between cases through lru_cache: never changed
    return a


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _launch(dev_scores, k, low_first):
    """One top-k twice on the same device tensor: (idx, val) as numpy, identical bits both times."""
    i1, v1 = _frt.topk(dev_scores, k, low_first)
    i2, v2 = _frt.topk(dev_scores, k, low_first)
    i1, v1, i2, v2 = (t.cpu().numpy() for t in (i1, v1, i2, v2))
    assert np.array_equal(i1, i2) and np.array_equal(_bits(v1), _bits(v2)), "two launches differ"
    return i1, v1


def _check(s, k, low_first, dev_scores=None):
    idx, val = _launch(torch.tensor(s, device=DEV) if dev_scores is None else dev_scores, k, low_first)
    ri, rv = ref_topk(s, k, low_first)
    bad = np.flatnonzero((idx != ri).any(1) | (_bits(val) != _bits(rv)).any(1))
    assert bad.size == 0, f"rows {bad.tolist()}: got idx {idx[bad[0]].tolist()} val {val[bad[0]].tolist()}, " \
                          f"want idx {ri[bad[0]].tolist()} val {rv[bad[0]].tolist()}"
    return idx, val


# ------------------------------------------------------------------ the seam grid
@functools.lru_cache(maxsize=None)
def _grid_rows(G):
    """9 rows (not a multiple of topk_kernel's 4 rows per block: its last block returns on row >= n)."""
    rng = np.random.default_rng(1000 + G)
    s = rng.random((9, G), dtype=np.float32)
    s[0] = 0.5                                                   # all equal: index order alone
    s[1] = np.where(rng.random(G) < 0.3, 0.75, 0.25)             # exactly 2 distinct values
    s[2] = 0.25
    s[2, rng.choice(G, 3, replace=False)] = 0.75                 # ... the higher one 3 times: fewer than most k
    s[3] = np.floor(s[3] * 8) / 8                                # 8 levels: ties at every rank
    s[4] = -s[4]                                                 # negative scores
    s[5, G - 1] = s[5, 0] = 2.0                                  # a two-way tie at the top, at the row's ends
    s[6] = np.where(rng.random(G) < 0.5, 0.0, -0.0)              # equal scores of different bits
    s[7, rng.choice(G, min(G, 5), replace=False)] = [INF, -INF, NAN, INF, -INF][:min(G, 5)]
    return _frozen(s)


@ORDERS
@pytest.mark.parametrize("k", [1, 7, 8, 9, 16])
@pytest.mark.parametrize("G", [16, 255, 256, 257, 1024, 1028])
def test_topk_seam_grid(G, k, low_first):
    """k on both sides of the 8 / 9 kernel switch and G on both sides of one pass of the small
    kernel's 256 threads (G = 16: most threads own nothing; 255 / 257: scalar loads; 256, 1024,
    1028: float4 loads, 1028 with a last group only thread 0 reads)."""
    _check(_grid_rows(G), k, low_first)


# ------------------------------------------------------------------ one thread owns the best
OWNER = 5          # the thread of the small kernel that gets all the planted entries
LAYOUTS = {
    # scalar loads (G % 4 != 0): thread t reads indices t, t + 256, ...
    "scalar": (2307, [OWNER + 256 * j for j in range(9)], 1000, False),
    # float4 loads: thread t reads elements 4g .. 4g + 3 of groups g = t, t + 256, t + 512
    "vector": (2304, [4 * g + e for g in (OWNER, OWNER + 256, OWNER + 512) for e in range(4)][:9], 1000, False),
    # G % 4 == 0 but the rows start 4 bytes into the buffer: the scalar fallback of the float4 test
    "offset": (2304, [OWNER + 256 * j for j in range(9)], 1000, True),
}


@functools.lru_cache(maxsize=None)
def _owner_rows(layout):
    G, pos, other, _ = LAYOUTS[layout]
    assert all(p < G for p in pos) and other not in pos
    rng = np.random.default_rng(7)
    s = rng.random((9, G), dtype=np.float32)                     # everything else is below 1
    shuffle = [3, 7, 0, 5, 8, 1, 6, 2, 4]
    r = 0
    for m in (8, 9):                                             # 9: one planted entry must be evicted
        asc = 2.0 + np.arange(m, dtype=np.float32) / 16
        for vals in (asc, asc[::-1], asc[[j for j in shuffle if j < m]]):   # in the thread's arrival order
            s[r, pos[:m]] = vals
            r += 1
    s[6, pos[:8]] = 2.0                                          # the owner's whole list is one tie
    s[7, pos[:9]] = 2.0                                          # ... and one of the tie does not fit
    s[8, pos[:8]] = 2.0 + np.arange(8, dtype=np.float32) / 16
    s[8, other] = 3.0                                            # the best elsewhere, the next 8 with the owner
    return _frozen(s)


@ORDERS
@pytest.mark.parametrize("k", [1, 7, 8, 9])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_topk_one_owner(layout, k, low_first):
    """The 8 (or 9) largest scores of a row all fall to one thread of the small kernel, arriving in
    ascending, descending and shuffled order: its 8-deep list is full, is popped k times, and with 9
    has dropped the right one.  (k = 9 runs topk_kernel on the same rows.)"""
    G, _pos, _other, offset = LAYOUTS[layout]
    s = _owner_rows(layout)
    if not offset:
        _check(s, k, low_first)
        return
    buf = torch.zeros(1 + s.size + 3, dtype=torch.float32, device=DEV)
    view = buf[1:1 + s.size].view(9, G)
    view.copy_(torch.tensor(s))
    assert view.data_ptr() % 16 == 4
    _check(s, k, low_first, dev_scores=view)


# ------------------------------------------------------------------ NaN, +-inf and short rows
@functools.lru_cache(maxsize=None)
def _special_rows(G, k):
    rng = np.random.default_rng(100 * G + k)
    s = rng.random((9, G), dtype=np.float32)

    def only(row, count, fill=NAN):
        """Leave `count` entries of the row, the rest := fill; returns the kept columns."""
        keep = rng.choice(G, count, replace=False)
        mask = np.ones(G, bool)
        mask[keep] = False
        s[row, mask] = fill
        return keep

    only(0, 0)                                                   # nothing rankable: k pads
    only(1, k - 1)                                               # one short
    only(2, k)                                                   # exactly k
    only(3, min(k + 1, G))                                       # one to spare
    s[4] = -INF                                                  # all -inf: real entries that look like pads
    keep = only(5, min(k + 1, G), fill=-INF)                     # the finite few above a floor of -inf
    s[5, keep[:2]] = INF                                         # a tie at +inf
    keep = only(6, k - 1)
    s[6, keep] = -INF                                            # k - 1 real -inf entries, then pads
    sprinkle = rng.choice(G, min(G, 12), replace=False)
    s[7, sprinkle] = np.resize(np.array([NAN, INF, -INF], np.float32), sprinkle.size)
    s[8] = np.where(rng.random(G) < 0.5, NAN, np.floor(s[8] * 4) / 4)   # half NaN, the rest tied
    return _frozen(s)


@ORDERS
@pytest.mark.parametrize("k", [1, 7, 8, 9, 16])
@pytest.mark.parametrize("G", [17, 256, 1028])
def test_topk_nan_inf_and_short_rows(G, k, low_first):
    """Rows whose rankable (non-NaN) count is 0, k - 1, k and k + 1, an all -inf row, +inf ties, and
    real -inf entries ahead of the padding: NONE -> idx -1 and the FIRST / NONE sentinels of both
    kernels."""
    _check(_special_rows(G, k), k, low_first)


# ------------------------------------------------------------------ rows that start off 16-byte alignment
@ORDERS
@pytest.mark.parametrize("k", [1, 8, 9])
def test_topk_unaligned_view_equals_aligned_copy(k, low_first):
    G = 1024
    s = _grid_rows(G)
    buf = torch.zeros(2 + 9 * G, dtype=torch.float32, device=DEV)
    view = buf.flatten()[1:1 + 9 * G].view(9, G)
    view.copy_(torch.tensor(s))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = _check(s, k, low_first, dev_scores=view)
    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0
    want = _launch(aligned, k, low_first)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


# ------------------------------------------------------------------ k = G: the whole row, sorted
@ORDERS
@pytest.mark.parametrize("G", [1, 8, 64])
def test_topk_whole_row(G, low_first):
    rng = np.random.default_rng(G)
    s = rng.random((9, G), dtype=np.float32)
    s[0] = 0.5
    s[1] = np.floor(s[1] * 4) / 4
    s[2, G // 2] = NAN                                           # k = G with one entry that never ranks
    idx, _ = _check(s, G, low_first)
    assert sorted(idx[3].tolist()) == list(range(G))


def test_reference_is_topk_policy_on_tied_rows():
    """ref_topk with the high index first is oracle.reference_path.topk_policy (the rule the rest of
    the suite holds the gallery search to) wherever that one is defined: NaN-free rows."""
    from oracle.reference_path import topk_policy
    s = _grid_rows(257)[:7]                                      # ties of every kind, no NaN
    assert not np.isnan(s).any()
    for k in (1, 8, 9, 257):
        ri, rv = ref_topk(s, k, False)
        pi, pv = topk_policy(s, k)
        assert np.array_equal(ri, pi) and np.array_equal(_bits(rv), _bits(pv))
    _check(s, 9, False)
