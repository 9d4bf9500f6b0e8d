"""GPU: ``fr_identity_scores`` and ``fr_eval_probes`` against the reference's results
(tests/golden/evaluate.npz) and against the host statements of their contracts
(``identity_scores_host`` / ``eval_probes_host``); their torch ops; the ``evaluate_*`` functions of
``evaluate_models`` on the device, end to end.  Cases, tolerances and margins: tests/_eval_cases.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _eval_cases as EC

pytestmark = pytest.mark.gpu

CASES = EC.all_cases()
f32 = np.float32


@pytest.fixture(scope="module")
def handle():
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=1)  # never finalised


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "evaluate.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scores(handle, Q, E, offsets, agg, k):
    out, sim = handle.identity_scores(_dev(Q), _dev(E), offsets, agg, k, return_sim=True)
    assert out.dtype == torch.float32 and sim.dtype == torch.float32 and out.is_cuda and sim.is_cuda
    return out.cpu().numpy(), sim.cpu().numpy()


# ---------------------------------------------------------------- fr_identity_scores
@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_identity_scores_match_the_reference(handle, fx, case):
    label = case["label"]
    exact = label.startswith("exact")
    names, Q = EC.pack(case["positive"]["all"])
    _m, NQ = EC.pack(case["negative"])
    _g, E = EC.pack(case["gallery"])
    offsets = EC.offsets_of(case["gallery"])
    tid = EC.true_ids(names, case["gallery"])
    assert EC.case_sha(case) == str(fx[f"{label}__sha256"])
    both = np.concatenate([Q, NQ])
    want_sim = np.concatenate([fx[f"{label}__sim"], fx[f"{label}__neg_sim"]])
    for agg, k in case["runs"]:
        pre = f"{label}__{agg}{k}__"
        want = np.concatenate([fx[pre + "scores"], fx[pre + "neg_scores"]])
        out, sim = _scores(handle, both, E, offsets, agg, k)
        print(pre, "max |out - ref|", np.abs(out - want).max(), "max |sim - ref|", np.abs(sim - want_sim).max())
        if exact:
            assert out.tobytes() == want.tobytes() and sim.tobytes() == want_sim.tobytes(), pre
        else:
            # the reference's own numbers keep every decision MARGIN away from a tie or a threshold
            EC.check_margins(fx[pre + "scores"], tid, fx[pre + "neg_scores"], fx[f"{label}__thresholds"],
                             EC.float64_scores(Q, E, offsets, agg, k), EC.float64_scores(NQ, E, offsets, agg, k))
            assert np.abs(out - want).max() <= EC.SCORE_TOL and np.abs(sim - want_sim).max() <= EC.SCORE_TOL, pre
        # without the sim output the scores live in the handle's workspace: the same result
        alone = handle.identity_scores(_dev(both), _dev(E), offsets, agg, k).cpu().numpy()
        assert alone.tobytes() == out.tobytes(), pre
    for k in case.get("topk_only", ()):
        out, _sim = _scores(handle, Q, E, offsets, "topk", k)
        assert np.abs(out - fx[f"{label}__topk{k}__scores_only"]).max() <= EC.SCORE_TOL, k


# identity lengths across 1..1024, more than EVAL_TILE_ROWS rows and more than EVAL_TILE_IDS identities
# in a row, so the aggregation kernel cuts tiles by rows and by identities
LENGTHS = ([1, 1, 2, 3, 8, 40, 63, 64, 65, 255, 256, 257, 1023, 1024, 1, 5] + [40] * 30 + [1] * 1100 +
           [8] * 20 + [1024, 1024, 1024, 1024, 1, 1000, 7])


@pytest.fixture(scope="module")
def batch():
    r = np.random.Generator(np.random.PCG64(0xE7A1_0010))
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    G = int(offsets[-1])
    cent = r.standard_normal((len(LENGTHS), 512))
    E = np.repeat(cent, LENGTHS, axis=0) + 0.8 * r.standard_normal((G, 512))
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(f32)
    E[r.choice(G, 50, replace=False)] *= f32(1.7)  # off-unit gallery rows
    Q = cent[r.integers(0, len(LENGTHS), 300)] + 0.9 * r.standard_normal((300, 512))
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(f32)
    Q[::7] *= f32(0.6)  # off-unit probes
    return Q, E, offsets


def _ulp_diff(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check_against_host(out, sim, offsets, agg, k):
    from facerecognitionpipeline_amd.evaluate_models import identity_scores_host
    want = identity_scores_host(sim, offsets, agg, k)
    if agg == "mean":  # one f32 ulp: the last rounding of a double sum taken in the same order
        assert (np.sign(out) == np.sign(want)).all() and _ulp_diff(out, want).max() <= 1, agg
    else:
        assert out.tobytes() == want.tobytes(), (agg, k)


@pytest.mark.parametrize("n", [1, 16, 17, 300])
def test_identity_scores_equal_the_host_statement(handle, batch, n):
    from facerecognitionpipeline_amd.evaluate_models import similarity_matrix_host
    Q, E, offsets = batch
    runs = [("max", 3), ("mean", 3), ("topk", 1), ("topk", 3), ("topk", 16)] if n in (17, 300) else \
        [("max", 3), ("mean", 3), ("topk", 3)]
    ref_sim = similarity_matrix_host(Q[:n], E)
    for agg, k in runs:
        out, sim = _scores(handle, Q[:n], E, offsets, agg, k)
        assert np.abs(sim - ref_sim).max() <= EC.SCORE_TOL
        _check_against_host(out, sim, offsets, agg, k)
    # a row's scores depend on nothing but that row: the first probe alone gives the same bits of out
    # for the sim it returns
    out1, sim1 = _scores(handle, Q[:1], E, offsets, "topk", 3)
    _check_against_host(out1, sim1, offsets, "topk", 3)


def test_identity_scores_chunk_seam(handle, batch):
    from facerecognitionpipeline_amd import _lib
    Q, E, offsets = batch
    L = _lib.load()
    L.frt_set_eval_chunk.restype = ctypes.c_int
    L.frt_set_eval_chunk.argtypes = [ctypes.c_int]
    whole = {a: _scores(handle, Q[:37], E, offsets, a, 3) for a in ("max", "mean", "topk")}
    assert L.frt_set_eval_chunk(16) == 0
    try:
        for agg, (out_w, sim_w) in whole.items():
            out, sim = _scores(handle, Q[:37], E, offsets, agg, 3)  # chunks of 16, 16 and 5 probes
            _check_against_host(out, sim, offsets, agg, 3)
            assert np.abs(sim - sim_w).max() <= EC.SCORE_TOL and np.abs(out - out_w).max() <= EC.SCORE_TOL
            alone = handle.identity_scores(_dev(Q[:37]), _dev(E), offsets, agg, 3).cpu().numpy()
            assert alone.tobytes() == out.tobytes()
    finally:
        assert L.frt_set_eval_chunk(0) == 0


def test_identity_scores_follow_the_precision_mode(fx):
    """The score GEMM runs in the handle's precision mode.  bf16x3 (x = hi + lo in bf16, three MFMAs per
    product) has a per-product relative error of about 2^-16 and the products of two rows of norm <= 1 sum to
    at most 1 in magnitude, so scores of unit rows stay within the conv kernels' 5e-5 bar of the reference
    (test_gpu_kernels.py); back in f32 the handle gives the f32 bits again."""
    from facerecognitionpipeline_amd import _lib
    h = _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=1)
    case = [c for c in CASES if c["label"] == "seeded"][0]
    _n, Q = EC.pack(case["positive"]["all"])
    _g, E = EC.pack(case["gallery"])
    offsets = EC.offsets_of(case["gallery"])
    want = fx["seeded__mean3__scores"]
    plain = _scores(h, Q, E, offsets, "mean", 3)[0]
    h.set_precision("bf16x3")
    try:
        fast = _scores(h, Q, E, offsets, "mean", 3)[0]
    finally:
        h.set_precision("fp32")
    print("bf16x3 max |out - ref|", np.abs(fast - want).max(), "f32", np.abs(plain - want).max())
    assert np.abs(fast - want).max() <= 5e-5 and np.abs(plain - want).max() <= EC.SCORE_TOL
    assert _scores(h, Q, E, offsets, "mean", 3)[0].tobytes() == plain.tobytes()


# ---------------------------------------------------------------- fr_eval_probes
def _probes(handle, scores, tid, thr):
    ri, rf, cnt = handle.eval_probes(_dev(scores), _dev(np.asarray(tid, np.int32)), thr)
    assert ri.dtype == torch.int32 and rf.dtype == torch.float32 and cnt.dtype == torch.int64
    return ri.cpu().numpy(), rf.cpu().numpy(), cnt.cpu().numpy()


def test_eval_probes_match_the_reference(handle, fx):
    for case in CASES:
        label = case["label"]
        if label == "norms":
            continue
        names, _Q = EC.pack(case["positive"]["all"])
        tid = EC.true_ids(names, case["gallery"])
        thr = fx[f"{label}__thresholds"]
        for agg, k in case["runs"]:
            pre = f"{label}__{agg}{k}__"
            ri, rf, cnt = _probes(handle, fx[pre + "scores"], tid, thr)  # the reference's matrix, as recorded
            assert np.array_equal(ri, fx[pre + "rec_i"]), pre
            assert rf.tobytes() == fx[pre + "rec_f"].tobytes(), pre
            assert np.array_equal(cnt, fx[pre + "counts"]), pre
            neg = fx[pre + "neg_scores"]
            ri, rf, cnt = _probes(handle, neg, np.full(len(neg), -1), thr)
            assert rf[:, 0].tobytes() == fx[pre + "ver_impostor"].tobytes(), pre
            assert np.array_equal(cnt[:, 2], fx[pre + "ver_table"][:, 6]), pre  # tn of the verification table


@pytest.mark.parametrize("n_ids", [1, 2, 64, 65, 300, 5000])
def test_eval_probes_equal_the_host_statement(handle, n_ids):
    from facerecognitionpipeline_amd.evaluate_models import eval_probes_host
    r = np.random.Generator(np.random.PCG64(0xE7A1_0020 + n_ids))
    n = 1000
    grid = np.linspace(-0.25, 0.95, 25).astype(f32)  # a small grid: equal scores are common
    cap = r.integers(3, 26, size=n)  # a cap of <= 5 leaves only scores below 0
    scores = grid[(r.integers(0, 1 << 30, size=(n, n_ids)) % cap[:, None])]
    tid = r.integers(0, n_ids, size=n).astype(np.int32)
    tid[::9] = -1
    tid[4::50] = n_ids
    tid[5::100] = np.iinfo(np.int32).max
    lead = np.arange(3, n, 8)  # some true identities lead alone, so rank 1 occurs among 5,000 tied columns too
    lead = lead[(tid[lead] >= 0) & (tid[lead] < n_ids)]
    scores[lead, tid[lead]] = f32(0.97)
    best = grid[:22]
    thr = np.concatenate([best.astype(np.float64), np.nextafter(best, f32(2)).astype(np.float64),
                          np.nextafter(best, f32(-2)).astype(np.float64), EC.NOTEBOOK_THRESHOLDS,
                          np.linspace(-0.3, 1.0, 175)])
    assert thr.shape == (256,)
    ri, rf, cnt = _probes(handle, scores, tid, thr)
    wi, wf, wc = eval_probes_host(scores, tid, thr)
    assert np.array_equal(ri, wi) and rf.tobytes() == wf.tobytes() and np.array_equal(cnt, wc)
    assert np.all(cnt[:, :3].sum(axis=1) == n)
    # what the batch has to contain
    enrolled = (tid >= 0) & (tid < n_ids)
    assert (~enrolled).sum() >= 100 and (ri[~enrolled, 2] == 0).all()
    assert (rf[:, 0] < 0).any() and (ri[rf[:, 0] < 0, 0] == -1).all()
    if n_ids > 1:
        srt = np.sort(scores, axis=1)
        assert (srt[:, -1] == srt[:, -2]).any()  # ties for the best score
        assert ((scores == rf[:, 1:2]).sum(axis=1)[enrolled] > 1).any()  # ties with the true identity
    ranks = ri[enrolled, 2]
    buckets = {1 if x == 1 else 5 if x <= 5 else 10 if x <= 10 else 11 for x in ranks}
    assert buckets == {b for b, lo in ((1, 1), (5, 2), (10, 6), (11, 11)) if n_ids >= lo}
    again = _probes(handle, scores, tid, thr)
    assert np.array_equal(again[0], ri) and again[1].tobytes() == rf.tobytes() and np.array_equal(again[2], cnt)


# ---------------------------------------------------------------- arguments, torch ops
def test_argument_errors_and_empty_batches(handle, batch):
    Q, E, offsets = batch
    q, e = _dev(Q[:4]), _dev(E)
    for off in ([1, 3], [0, 0, len(E)], [0, len(E)]):  # offsets[0] != 0, an empty identity, over 1024 rows
        with pytest.raises(ValueError):
            handle.identity_scores(q, e, off)
    with pytest.raises(ValueError):
        handle.identity_scores(q, e, offsets, "median")
    with pytest.raises(ValueError):
        handle.identity_scores(q, e, offsets, "topk", 0)
    with pytest.raises(NotImplementedError):
        handle.identity_scores(q, e, offsets, "topk", 17)
    with pytest.raises(ValueError):
        handle.identity_scores(q.cpu(), e, offsets)
    with pytest.raises(ValueError):
        handle.identity_scores(q.double(), e, offsets)
    with pytest.raises(ValueError):
        handle.identity_scores(q, e, offsets[:-1])  # offsets that do not end at the rows of E
    out, sim = handle.identity_scores(q[:0], e, offsets, return_sim=True)  # no probes: a no-op
    assert tuple(out.shape) == (0, len(offsets) - 1) and tuple(sim.shape) == (0, len(E))
    handle.identity_scores(q, e, offsets, "mean", 0)  # k is ignored by max and mean
    s = _dev(np.zeros((3, 5), f32))
    t = _dev(np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        handle.eval_probes(s, t, np.zeros(257))
    with pytest.raises(ValueError):
        handle.eval_probes(s, t.long(), [0.5])
    with pytest.raises(ValueError):
        handle.eval_probes(s.cpu(), t.cpu(), [0.5])
    with pytest.raises(ValueError):
        handle.eval_probes(s[:, :0], t, [0.5])
    ri, rf, cnt = handle.eval_probes(s[:0], t[:0], [0.2, 0.5])  # no probes: counts are zeroed
    assert tuple(ri.shape) == (0, 4) and tuple(rf.shape) == (0, 4) and cnt.cpu().tolist() == [[0] * 4] * 2
    ri, rf, cnt = handle.eval_probes(s, t, [])  # no thresholds: records only
    assert tuple(cnt.shape) == (0, 4) and ri.cpu().tolist() == [[0, 0, 1, 1]] * 3


def test_torch_ops(handle, batch):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    Q, E, offsets = batch
    q, e = _dev(Q[:20]), _dev(E)
    tid = _dev(np.arange(20, dtype=np.int32))
    thr = EC.NOTEBOOK_THRESHOLDS.tolist()
    for agg in ("max", "mean", "topk"):
        got = torch.ops.frhip.identity_scores(q, e, offsets.tolist(), agg, 3)
        want = handle.identity_scores(q, e, offsets, agg, 3)
        assert torch.equal(got, want)
        for a, b in zip(torch.ops.frhip.eval_probes(got, tid, thr), handle.eval_probes(want, tid, thr)):
            assert torch.equal(a, b)
    with FakeTensorMode():
        out = torch.ops.frhip.identity_scores(torch.empty(9, 512, device="cuda"), torch.empty(20, 512, device="cuda"),
                                              [0, 4, 9, 20], "topk", 3)
        assert out.shape == (9, 3) and out.dtype == torch.float32 and out.device.type == "cuda"
        ri, rf, cnt = torch.ops.frhip.eval_probes(out, torch.empty(9, dtype=torch.int32, device="cuda"), [0.2, 0.5])
        assert ri.shape == (9, 4) and rf.shape == (9, 4) and cnt.shape == (2, 4) and cnt.dtype == torch.int64


# ---------------------------------------------------------------- evaluate_* end to end
@pytest.mark.parametrize("label", ["seeded", "exact_n300", "exact_multi"])
def test_evaluate_functions_on_the_device(handle, fx, label):
    """The four evaluate_* functions on the device against the recorded reference results: rank metrics,
    predictions and table counts equal, scores and score statistics within 1e-6 (bit for bit on the exact
    cases), ROC-AUC, EER and TAR@FAR equal."""
    from facerecognitionpipeline_amd import evaluate_models as EM
    case = [c for c in CASES if c["label"] == label][0]
    for i, (agg, k) in enumerate(case["runs"]):
        engine = {"device": "cuda"} if i % 2 == 0 else {"handle": handle}
        EC.check_evaluate_functions(EM, fx, case, agg, k, **engine)


def test_topk_beyond_the_kernel_limit_takes_the_host_statement(handle):
    from facerecognitionpipeline_amd import evaluate_models as EM
    case = [c for c in CASES if c["label"] == "seeded"][0]
    thr = EC.NOTEBOOK_THRESHOLDS
    dev = EM.evaluate_probes_comprehensive(case["gallery"], case["positive"], thr, "topk", 20, handle=handle)
    host = EM.evaluate_probes_comprehensive(case["gallery"], case["positive"], thr, "topk", 20)
    assert dev["threshold_results"] == host["threshold_results"]
    assert [p["predicted_identity"] for p in dev["all_predictions"]] == \
        [p["predicted_identity"] for p in host["all_predictions"]]


def test_evaluate_with_the_synthetic_embedder():
    """8 identities x 2 gallery crops and 16 sigma-12 probes through the synthetic IR-50 embedder, built as
    test_gpu_track_consensus.py builds its tracks (there the CPU oracle scores every such probe at least
    0.9993 on its own row and 0.035 clear of the rest): rank-1 is 1.0 and the 'max' scores are within 1e-5 of
    the oracle's.  The oracle's own best-to-second margin is asserted to be 100 times that tolerance."""
    from facerecognitionpipeline_amd import evaluate_models as EM
    from facerecognitionpipeline_amd import weights as W
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    from oracle import reference_path as rp
    from oracle.adaface_net import load_oracle
    emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=64)
    base = W.synthetic_crops(8)

    def noisy(i, n, seed):
        return W.probe_crops(base[i:i + 1], n, sigma=12.0, seed=seed)

    second = np.concatenate([noisy(i, 1, 30 + i) for i in range(8)])
    probes = np.concatenate([noisy(i, 2, 50 + i) for i in range(8)])  # probes 2i, 2i + 1 of identity i
    crops = np.concatenate([base, second, probes])
    got = np.asarray(emb.extract_embeddings_batch(list(crops)), f32)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = np.asarray(rp.extract_embeddings_batch(load_oracle("ir_50", W.synthetic_state_dict("ir_50")), list(crops)), f32)

    def dicts(e):
        gallery = {f"S{i:03d}": {"embeddings": np.stack([e[i], e[8 + i]])} for i in range(8)}
        positive = {f"S{i:03d}": {"embeddings": e[16 + 2 * i:18 + 2 * i]} for i in range(8)}
        return gallery, positive

    gallery, positive = dicts(got)
    res = EM.evaluate_probes_comprehensive(gallery, positive, EC.NOTEBOOK_THRESHOLDS, aggregation="max",
                                           device=emb.device)
    assert len(res["all_predictions"]) == 16
    assert res["threshold_results"][0]["rank1_accuracy"] == 1.0 and res["threshold_results"][0]["mrr"] == 1.0
    assert all(p["predicted_identity"] == p["true_identity"] for p in res["all_predictions"])
    ogallery, opositive = dicts(ref)
    want = EM.evaluate_probes_comprehensive(ogallery, opositive, EC.NOTEBOOK_THRESHOLDS, aggregation="max")
    for p, w in zip(res["all_predictions"], want["all_predictions"]):
        print("score", float(p["score"]), "oracle", float(w["score"]))
        assert abs(float(p["score"]) - float(w["score"])) <= 1e-5
        others = [v for g, v in w["identity_scores"].items() if g != w["true_identity"]]
        assert w["predicted_identity"] == w["true_identity"] and float(w["score"]) - float(max(others)) >= 1e-3
