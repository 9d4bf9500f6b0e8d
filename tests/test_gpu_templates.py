"""template_kernel (gallery.hip) on planted students: the quality filter's threshold and tie rules,
the sample limit, the median's rank tie-break and weighted_mean on two rows.

Every sample row here has dyadic entries (four of +-1/2, or sixty-four of +-1/8), so each dot product
of two rows and each row sum of the Gram matrix is exact in float32 whatever the order of the
reduction.  avg_i = (row sum) / N is then ONE correctly rounded float32 division on the device and in
the restatement below, the filter's decisions have no rounding slack and `kept` is compared exactly.
Which rows were kept shows in the template: the rows have private dimensions, and a template built
from other rows is off by far more than the tolerance.

The templates are held to a float64 restatement of GalleryManager._aggregate_embeddings at the
tolerances of test_gpu_gallery.py's random test: 1e-7 for mean, 1e-6 for median and weighted_mean.
The restatement's fallback is np.argsort(avg, kind="stable")[-2:]: the reference's default argsort
leaves the order of equal averages undefined (oracle/reference_path.py: topk_policy), the kernel fixes
it to the stable sort's, and these cases are all about equal averages.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
METHODS = ["mean", "median", "weighted_mean"]
TOL = {"mean": 1e-7, "median": 1e-6, "weighted_mean": 1e-6}
f32 = np.float32


@pytest.fixture(scope="module")
def handle():
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=1)


# ------------------------------------------------------------------ rows
def quad(dims, signs=(1, 1, 1, 1), value=0.5):
    r = np.zeros(512, f32)
    r[list(dims)] = value * np.asarray(signs, f32)
    return r


def block(i):
    """Row i of a set of mutually orthogonal unit rows: +1/2 on dimensions 4i .. 4i + 3."""
    return quad(range(4 * i, 4 * i + 4))


def family(i):
    """Row i of a set with pairwise dot exactly 0.75: +1/2 on dimensions 0, 1, 2 and on 3 + i."""
    return quad((0, 1, 2, 3 + i))


# ------------------------------------------------------------------ the restatement
def stable_filter(E, min_similarity):
    """Indices _filter_quality_embeddings keeps (gallery_manager.py:104-122), in row order, with a
    stable argsort in the fallback; avg in float32 from exact row sums."""
    N = len(E)
    if N <= 2:
        return np.arange(N)
    E64 = E.astype(np.float64)
    sims = E64 @ E64.T
    assert np.array_equal(sims, (E @ E.T).astype(np.float64)), "the Gram matrix is not exact in float32"
    np.fill_diagonal(sims, 0)
    sums = sims.sum(axis=1)
    assert np.array_equal(sums, sums.astype(f32).astype(np.float64))
    avg = sums.astype(f32) / f32(N)
    keep = np.flatnonzero(avg >= f32(min_similarity))
    if len(keep) < 2:
        keep = np.sort(np.argsort(avg, kind="stable")[-2:])
    return keep


def template64(E, keep, method):
    """_aggregate_embeddings (gallery_manager.py:297-317) of the kept rows in float64."""
    e = E[keep].astype(np.float64)
    if method == "median":
        agg = np.median(e, axis=0)
    elif method == "weighted_mean":
        w = np.mean(e @ e.T, axis=1)
        w = w / np.sum(w)
        agg = np.sum(e * w[:, None], axis=0)
    else:
        agg = np.mean(e, axis=0)
    return agg / (np.linalg.norm(agg) + 1e-8)


def run(handle, students, method, min_similarity=0.70, want_keep=None):
    """Build the templates of `students` (a list of [N_i,512] arrays) in one CSR call and hold every
    one to the restatement.  want_keep: {student: kept rows} the case was planted for."""
    sizes = [len(e) for e in students]
    off = np.concatenate([[0], np.cumsum(sizes)])
    emb = torch.from_numpy(np.concatenate(students)).cuda()
    tpl, kept = handle.build_templates(emb, off, method, min_similarity)
    tpl, kept = tpl.cpu().numpy(), kept.cpu().numpy()
    for i, E in enumerate(students):
        if len(E) == 1:
            assert kept[i] == 1 and np.array_equal(tpl[i].view(np.int32), E[0].view(np.int32)), i
            continue
        keep = stable_filter(E, min_similarity)
        if want_keep is not None and i in want_keep:
            assert keep.tolist() == list(want_keep[i]), (i, keep.tolist())   # the case is what it was planted as
        assert kept[i] == len(keep), (i, int(kept[i]), keep.tolist())
        d = np.abs(tpl[i] - template64(E, keep, method)).max()
        assert d <= TOL[method], (i, len(E), method, d)
    return tpl, kept


def next_up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


# ------------------------------------------------------------------ the fallback's tie rule
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [3, 20])
def test_fallback_all_averages_equal_keeps_the_last_two(handle, method, N):
    """N mutually orthogonal rows: every avg is 0, nothing reaches 0.70, and the fallback's N-way tie
    keeps rows N - 2 and N - 1, as np.argsort(avg, kind="stable")[-2:] does."""
    E = np.stack([block(i) for i in range(N)])
    run(handle, [E], method, want_keep={0: [N - 2, N - 1]})


@pytest.mark.parametrize("method", METHODS)
def test_fallback_when_exactly_one_row_passes(handle, method):
    """avg = (1/3, 1/6, 1/6): only row 0 reaches 0.3, so c == 1 and the top two are taken instead:
    row 0 and, of the tied rows 1 and 2, the later one."""
    E = np.stack([quad((0, 1, 2, 3)), quad((0, 1, 4, 5)), quad((2, 3, 6, 7))])
    run(handle, [E], method, min_similarity=0.3, want_keep={0: [0, 2]})


# ------------------------------------------------------------------ avg == min_similarity
def _threshold_students():
    """(rows, the family rows' avg): a family with pairwise dot 0.75 among orthogonal strangers."""
    four = np.stack([family(0), family(1), block(100), family(2)])              # avg = 1.5 / 4 = 0.375
    ten = np.stack([block(100 + i) if i in (0, 3, 4, 6, 8, 9) else family(i) for i in range(10)])
    return (four, float(f32(1.5) / f32(4))), (ten, float(f32(2.25) / f32(10)))  # ten: 4 family rows, 0.225f


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("which", [0, 1], ids=["N4_avg_0.375", "N10_avg_0.225f"])
def test_row_at_the_threshold_is_kept_and_one_ulp_above_it_is_dropped(handle, method, which):
    E, avg = _threshold_students()[which]
    fam = [i for i in range(len(E)) if E[i, 0] != 0]
    # avg >= min_similarity with equality, bit for bit: the whole family stays
    run(handle, [E], method, min_similarity=avg, want_keep={0: fam})
    # the threshold one float32 step higher: nobody passes, and the fallback takes the last two of the tie
    run(handle, [E], method, min_similarity=next_up(avg), want_keep={0: fam[-2:]})


# ------------------------------------------------------------------ N = 1, N = 2
@pytest.mark.parametrize("method", METHODS)
def test_one_and_two_samples(handle, method):
    """N = 1: the row itself, not normalised (planted with norm 2).  N = 2: no filter, whatever the
    similarity (orthogonal rows; rows of norm 1 and 2 with dot 1, so weighted_mean's two weights
    differ: (1 + 1) / 2 and (1 + 4) / 2 before they are normalised)."""
    single = quad((9, 200, 300, 511), (1, -1, 1, -1), value=1.0)[None]
    assert np.linalg.norm(single[0]) == 2.0
    pair = np.stack([block(1), block(0)])
    uneven = np.stack([quad((0, 1, 2, 3)), quad((0, 1, 4, 5), value=1.0)])
    _tpl, kept = run(handle, [single, pair, uneven, single], method, want_keep={1: [0, 1], 2: [0, 1]})
    assert kept.tolist() == [1, 2, 2, 1]


# ------------------------------------------------------------------ the sample limit
@functools.lru_cache(maxsize=None)
def _limit_students(N):
    """A student of N samples between a student of 1 and a student of 3 (a stride slip at the limit
    lands in a neighbour).  Rows of sixty-four +-1/8: seven of eight share dimensions 0..59 and carry
    4 private ones (pairwise dot >= 56/64: kept), every eighth lives on dimensions 448..511 alone
    (orthogonal to the others, +-small among themselves: dropped)."""
    rng = np.random.default_rng(N)
    E = np.zeros((N, 512), f32)
    for i in range(N):
        if i % 8 == 5:
            E[i, 448:] = rng.choice([-0.125, 0.125], 64)
        else:
            E[i, :60] = 0.125
            E[i, rng.choice(np.arange(60, 448), 4, replace=False)] = rng.choice([-0.125, 0.125], 4)
    before = quad((9, 200, 300, 511), value=1.0)[None]
    after = np.stack([block(7), block(8), block(9)])
    for a in (E, before, after):
        a.setflags(write=False)
    return [before, E, after]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [1023, 1024])
def test_sample_limit_between_neighbours(handle, method, N):
    students = _limit_students(N)
    dropped = [i for i in range(N) if i % 8 == 5]
    keep = [i for i in range(N) if i % 8 != 5]
    _tpl, kept = run(handle, students, method, want_keep={1: keep, 2: [1, 2]})
    assert kept.tolist() == [1, N - len(dropped), 2]


# ------------------------------------------------------------------ the median's ranks
@pytest.mark.parametrize("order", ["AB", "AA", "ABA", "AAB", "AABC", "ABAB", "ABACB", "AAAAB", "CBAAA"])
def test_median_with_duplicated_rows(handle, order):
    """2..5 kept rows with repeats (min_similarity far below any avg: every row passes), values from
    {-1/2, 0, 1/2} so that most columns hold equal values and the rank's b < a tie-break places
    them; two columns are equal in every row."""
    rng = np.random.default_rng(5)
    rows = {c: rng.choice(np.array([-0.5, 0.0, 0.5], f32), 512) for c in "ABC"}
    E = np.stack([rows[c] for c in order])
    E[:, 7], E[:, 8] = 0.5, -0.5
    run(handle, [E], "median", min_similarity=-1e30, want_keep={0: range(len(order))})


# ------------------------------------------------------------------ kept is optional
def test_templates_without_kept(handle):
    """fr_build_templates with kept == NULL (include/frhip.h) writes the same templates."""
    from facerecognitionpipeline_amd import _lib
    students = [np.stack([block(i) for i in range(3)]), quad((1, 2, 3, 4), value=1.0)[None],
                np.stack([family(i) for i in range(16)])]                    # avg = 0.75 * 15 / 16: all kept
    off = np.concatenate([[0], np.cumsum([len(e) for e in students])]).astype(np.int32)
    emb = torch.from_numpy(np.concatenate(students)).cuda()
    want, kept = handle.build_templates(emb, off, "mean")
    assert kept.cpu().numpy().tolist() == [2, 1, 16]
    got = torch.full_like(want, float("nan"))
    _lib.check(_lib.load().fr_build_templates(handle.h, emb.data_ptr(), off.ctypes.data, 3, 0, ctypes.c_float(0.70),
                                              got.data_ptr(), None, torch.cuda.current_stream().cuda_stream),
               handle.h)
    assert torch.equal(got, want)
