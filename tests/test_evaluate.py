"""CPU: the host statements of fr_identity_scores / fr_eval_probes and the reference-named functions of
facerecognitionpipeline_amd.evaluate_models against the reference's own results in
tests/golden/evaluate.npz (tools/make_golden.py evaluate); the two C calls' argument errors; the
torch ops' fake implementations."""
import ctypes
import os

import numpy as np
import pytest

from tests import _eval_cases as EC

CASES = EC.all_cases()
RUNS = [(c, agg, k) for c in CASES for agg, k in c["runs"]]
RUN_IDS = [f"{c['label']}-{agg}{k}" for c, agg, k in RUNS]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "evaluate.npz"))


def test_cases_are_the_recorded_ones(fx):
    assert fx["labels"].tolist() == [c["label"] for c in CASES]
    for c in CASES:
        assert EC.case_sha(c) == str(fx[f"{c['label']}__sha256"]), c["label"]
        assert np.array_equal(EC.thresholds_of(c), fx[f"{c['label']}__thresholds"])


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_similarity_matrix_host(fx, case):
    from facerecognitionpipeline_amd import evaluate_models as EM
    _n, Q = EC.pack(case["positive"]["all"])
    _m, NQ = EC.pack(case["negative"])
    _g, E = EC.pack(case["gallery"])
    for q, name in ((Q, "sim"), (NQ, "neg_sim")):
        got, want = EM.similarity_matrix_host(q, E), fx[f"{case['label']}__{name}"]
        if case["label"].startswith("exact"):
            assert got.tobytes() == want.tobytes()
        else:
            assert np.abs(got - want).max() <= EC.SCORE_TOL
    # the pairwise function is the same rule
    pairs = EM.compute_all_similarities(Q[0], case["gallery"])
    assert [n for n, _s in pairs] == [n for n, v in case["gallery"].items() for _ in v["embeddings"]]
    assert np.abs(np.array([s for _n, s in pairs], np.float32) - fx[f"{case['label']}__sim"][0]).max() <= EC.SCORE_TOL
    assert abs(EM.cosine_similarity(Q[0], E[0]) - fx[f"{case['label']}__sim"][0, 0]) <= EC.SCORE_TOL


@pytest.mark.parametrize("case,agg,k", RUNS, ids=RUN_IDS)
def test_host_statements_against_the_reference(fx, case, agg, k):
    from facerecognitionpipeline_amd import evaluate_models as EM
    label = case["label"]
    pre = f"{label}__{agg}{k}__"
    names, _Q = EC.pack(case["positive"]["all"])
    tid = EC.true_ids(names, case["gallery"])
    offsets = EC.offsets_of(case["gallery"])
    got = EM.identity_scores_host(fx[f"{label}__sim"], offsets, agg, k)  # on the reference's own sim
    if label.startswith("exact"):
        assert got.tobytes() == fx[pre + "scores"].tobytes()
    else:
        assert np.abs(got - fx[pre + "scores"]).max() <= EC.SCORE_TOL
        EC.check_margins(fx[pre + "scores"], tid, fx[pre + "neg_scores"], fx[f"{label}__thresholds"])
    # the records and counts of the reference's own score matrix: bit for bit, ints included
    rec_i, rec_f, counts = EM.eval_probes_host(fx[pre + "scores"], tid, fx[f"{label}__thresholds"])
    assert rec_i.dtype == np.int32 and rec_f.dtype == np.float32 and counts.dtype == np.int64
    assert np.array_equal(rec_i, fx[pre + "rec_i"])
    assert rec_f.tobytes() == fx[pre + "rec_f"].tobytes()
    assert np.array_equal(counts, fx[pre + "counts"])
    assert np.all(counts[:, :3].sum(axis=1) == len(names))


@pytest.mark.parametrize("case,agg,k", RUNS, ids=RUN_IDS)
def test_evaluate_functions_against_the_reference(fx, case, agg, k):
    from facerecognitionpipeline_amd import evaluate_models as EM
    EC.check_evaluate_functions(EM, fx, case, agg, k)


def test_identify_probe_and_topk_k(fx):
    from facerecognitionpipeline_amd import evaluate_models as EM
    case = [c for c in CASES if c["label"] == "seeded"][0]
    names, Q = EC.pack(case["positive"]["all"])
    gnames = list(case["gallery"])
    _g, E = EC.pack(case["gallery"])
    sim = EM.similarity_matrix_host(Q, E)
    for k in case["topk_only"]:
        want = fx[f"seeded__topk{k}__scores_only"]
        assert np.abs(EM.identity_scores_host(sim, EC.offsets_of(case["gallery"]), "topk", k) - want).max() <= EC.SCORE_TOL
        name, score, scores = EM.identify_probe(Q[5], case["gallery"], 0.0, "topk", k)
        assert list(scores) == gnames and name == gnames[int(np.argmax(want[5]))]
        assert abs(score - want[5].max()) <= EC.SCORE_TOL
        assert EM.compute_rank_metrics(scores, names[5]) == EM._rank_metrics_of(
            1 + sorted(scores, key=scores.get, reverse=True).index(names[5]))
    # a large k is every row: the mean
    big = EM.identity_scores_host(sim, EC.offsets_of(case["gallery"]), "topk", 5000)
    assert np.abs(big - EM.identity_scores_host(sim, EC.offsets_of(case["gallery"]), "mean")).max() <= 2e-7
    assert EM.identify_probe(Q[0], case["gallery"], 2.0, "max")[0] is None
    assert EM.identify_probe(Q[0], {}, 0.0) == (None, -1, {})
    assert EM.compute_rank_metrics({"a": 0.5, "b": 0.5, "c": 0.1}, "b") == {
        "rank1": False, "rank5": True, "rank10": True, "reciprocal_rank": 0.5}
    assert EM.compute_rank_metrics({"a": 0.5}, "zz")["reciprocal_rank"] == 0.0
    assert EM.aggregate_max([]) == -1 and EM.aggregate_mean([]) == -1 and EM.aggregate_topk([]) == -1
    assert EM.aggregate_max([0.25, 0.5]) == 0.5 and EM.aggregate_mean([0.25, 0.5]) == 0.375
    assert EM.aggregate_topk([0.25, 0.5, 0.75, 0.125], k=2) == 0.625
    assert EM.compute_dprime([], [0.1]) == 0.0 and EM.compute_dprime([0.5, 0.5], [0.5, 0.5]) == 0.0


def test_bootstrap_confidence_interval(fx):
    from facerecognitionpipeline_amd import evaluate_models as EM
    data = fx["bootstrap_data"].tolist()
    np.random.seed(1234)  # rng=None draws from numpy's global generator, as the reference does
    assert EM.bootstrap_confidence_interval(data, n_bootstrap=200) == tuple(fx["bootstrap_ci_seed1234_n200"])
    a = EM.bootstrap_confidence_interval(data, n_bootstrap=50, rng=np.random.default_rng(3))
    b = EM.bootstrap_confidence_interval(data, n_bootstrap=50, rng=np.random.default_rng(3))
    assert a == b and a[0] < np.mean(data) < a[1]
    assert EM.bootstrap_confidence_interval([]) == (0.0, 0.0)


def test_input_checks():
    from facerecognitionpipeline_amd import evaluate_models as EM
    good = np.zeros((2, 512), np.float32)
    good[:, 0] = 1
    for bad in (np.full((1, 512), np.nan, np.float32), np.zeros((1, 512), np.float32)):
        with pytest.raises(ValueError):
            EM.pack_gallery({"a": {"embeddings": bad}})
        with pytest.raises(ValueError):
            EM.evaluate_impostors_comprehensive({"a": {"embeddings": good}}, {"x": {"embeddings": bad}}, [0.5])
    with pytest.raises(ValueError):
        EM.identity_scores_host(np.zeros((1, 3), np.float32), [0, 2], "mean")
    with pytest.raises(ValueError):
        EM.identity_scores_host(np.zeros((1, 3), np.float32), [0, 3], "median")
    with pytest.raises(ValueError):  # no genuine score: the probe's name is not enrolled
        EM.evaluate_verification_comprehensive({"a": {"embeddings": good}}, {"b": {"embeddings": good}},
                                               {"x": {"embeddings": good}}, [0.5])
    g = EM.pack_gallery({"a": {"embeddings": good}})
    assert EM.pack_gallery(g) is g and g.offsets.tolist() == [0, 2] and "a" in g


def test_argument_errors_without_gpu():
    """The argument checks of both calls come before the handle, so they are reported for a NULL handle."""
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    q = (ctypes.c_float * 1024)()
    e = (ctypes.c_float * 4096)()
    out = (ctypes.c_float * 16)()
    INV, UNS = _lib.FR_ERR_INVALID_ARGUMENT, _lib.FR_ERR_UNSUPPORTED

    def scores(Q=q, n=2, E=e, offsets=(0, 3, 8), n_ids=2, agg=1, k=3, out=out):
        off = (ctypes.c_int32 * len(offsets))(*offsets) if offsets is not None else None
        rc = lib.fr_identity_scores(None, Q, n, E, off, n_ids, agg, k, out, None, None)
        return rc, lib.fr_last_error(None)

    for kw, code, text in (({}, INV, b"NULL handle"), ({"n": 0}, INV, b"NULL handle"),
                           ({"Q": None}, INV, b"NULL buffer"), ({"E": None}, INV, b"NULL buffer"),
                           ({"out": None}, INV, b"NULL buffer"), ({"offsets": None}, INV, b"NULL buffer"),
                           ({"n": -1}, INV, b"bad n"), ({"n_ids": 0}, INV, b"n_ids"),
                           ({"offsets": (1, 3, 8)}, INV, b"id_offsets[0]"),
                           ({"offsets": (0, 0, 8)}, INV, b"identity 0 has 0"),
                           ({"offsets": (0, 3, 2)}, INV, b"identity 1 has -1"),
                           ({"offsets": (0, 3, 3 + 1025)}, INV, b"identity 1 has 1025"),
                           ({"agg": 3}, INV, b"aggregation"), ({"agg": -1}, INV, b"aggregation"),
                           ({"agg": 2, "k": 0}, INV, b"k must be"), ({"agg": 2, "k": 17}, UNS, b"k <= 16"),
                           ({"agg": 1, "k": 0}, INV, b"NULL handle"), ({"agg": 0, "k": 99}, INV, b"NULL handle")):
        rc, msg = scores(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert float(out[0]) == 0.0  # nothing was written

    a = (ctypes.c_float * 16)()
    t = (ctypes.c_int32 * 4)()
    ri = (ctypes.c_int32 * 16)()
    rf = (ctypes.c_float * 16)()
    cnt = (ctypes.c_int64 * 8)()
    thr = (ctypes.c_double * 2)(0.3, 0.5)

    def probes(scores=a, n=4, n_ids=4, true_id=t, thr=thr, n_thr=2, ri=ri, rf=rf, cnt=cnt):
        rc = lib.fr_eval_probes(None, scores, n, n_ids, true_id, thr, n_thr, ri, rf, cnt, None)
        return rc, lib.fr_last_error(None)

    for kw, text in (({}, b"NULL handle"), ({"scores": None}, b"NULL buffer"), ({"true_id": None}, b"NULL buffer"),
                     ({"thr": None}, b"NULL buffer"), ({"ri": None}, b"NULL buffer"), ({"rf": None}, b"NULL buffer"),
                     ({"cnt": None}, b"NULL buffer"), ({"n": -1}, b"n must be"), ({"n_ids": 0}, b"n_ids"),
                     ({"n_thr": -1}, b"n_thr"), ({"n_thr": 257}, b"n_thr"),
                     ({"n_thr": 0, "thr": None, "cnt": None}, b"NULL handle")):
        rc, msg = probes(**kw)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT and text in msg, (kw, rc, msg)
    lib.frt_set_eval_chunk.restype = ctypes.c_int
    lib.frt_set_eval_chunk.argtypes = [ctypes.c_int]
    assert lib.frt_set_eval_chunk(-1) == _lib.FR_ERR_INVALID_ARGUMENT and lib.frt_set_eval_chunk(0) == 0


def test_op_shapes_without_gpu():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        q = torch.empty(9, 512)
        e = torch.empty(20, 512)
        out = torch.ops.frhip.identity_scores(q, e, [0, 4, 9, 20], "topk", 3)
        assert out.shape == (9, 3) and out.dtype == torch.float32
        ri, rf, cnt = torch.ops.frhip.eval_probes(out, torch.empty(9, dtype=torch.int32), [0.2, 0.5])
        assert ri.shape == (9, 4) and ri.dtype == torch.int32
        assert rf.shape == (9, 4) and rf.dtype == torch.float32
        assert cnt.shape == (2, 4) and cnt.dtype == torch.int64
    with pytest.raises(ValueError):  # CPU tensors: there is no CPU fallback
        torch.ops.frhip.identity_scores(torch.zeros(1, 512), torch.zeros(2, 512), [0, 2], "mean", 3)
    with pytest.raises(ValueError):
        torch.ops.frhip.eval_probes(torch.zeros(1, 2), torch.zeros(1, dtype=torch.int32), [0.5])
