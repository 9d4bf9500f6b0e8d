"""GPU: ``fr_samples_set`` / ``fr_match_identities`` / ``fr_embed_match_identities`` against the
notebook's recorded ``identify_probe`` scores (tests/golden/evaluate.npz) and the host statement
(``match_identities_host``), the fused and the composed path on the same inputs; tile and lane edges;
the handle's state; ``GalleryManager`` / ``FaceMatcher`` identity aggregation end to end.  Cases and
tolerances: tests/_eval_cases.py; the order rule: tests/_identity_cases.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _eval_cases as EC
from tests import _identity_cases as IC

pytestmark = pytest.mark.gpu

CASES = EC.all_cases()
f32 = np.float32
RULE, FUSED, COMPOSED = 0, 1, 2
SIGMA = 12.0


@pytest.fixture(scope="module")
def lib():
    from facerecognitionpipeline_amd import _lib
    L = _lib.load()
    for name in ("frt_set_identify_path", "frt_set_identify_tile_rows"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int]
    yield L
    assert L.frt_set_identify_path(RULE) == 0 and L.frt_set_identify_tile_rows(0) == 0


@pytest.fixture(scope="module")
def handle():
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=1)  # never finalised


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "evaluate.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _match(lib, handle, Q, agg, agg_k, k, path):
    """idx / score [n,k] of Q through ``path``: the fused kernel in chunks of at most 16 queries (what a
    serving caller sends), the composed path and the built-in rule on the whole batch."""
    n = len(Q)
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    score = torch.empty((n, k), dtype=torch.float32, device="cuda")
    step = 16 if path == FUSED else max(n, 1)
    assert lib.frt_set_identify_path(path) == 0
    try:
        for q0 in range(0, n, step):
            handle.match_identities(_dev(Q[q0:q0 + step]), agg, agg_k, k, idx[q0:q0 + step], score[q0:q0 + step])
    finally:
        assert lib.frt_set_identify_path(RULE) == 0
    return idx.cpu().numpy(), score.cpu().numpy()


def _ks(n_ids):
    return sorted({1, min(5, n_ids), n_ids})


# ---------------------------------------------------------------- the recorded reference
@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_match_identities_against_the_reference(lib, handle, fx, case):
    from facerecognitionpipeline_amd.evaluate_models import match_identities_host
    label = case["label"]
    exact = label.startswith("exact")
    _n, Q = EC.pack(case["positive"]["all"])
    _m, NQ = EC.pack(case["negative"])
    _g, E = EC.pack(case["gallery"])
    offsets = EC.offsets_of(case["gallery"])
    assert EC.case_sha(case) == str(fx[f"{label}__sha256"])
    n_ids = len(offsets) - 1
    handle.samples_set(_dev(E), offsets)
    assert handle.samples_size() == (n_ids, len(E))
    both = np.concatenate([Q, NQ])
    runs = [(agg, k, both, np.concatenate([fx[f"{label}__{agg}{k}__scores"], fx[f"{label}__{agg}{k}__neg_scores"]]))
            for agg, k in case["runs"]]
    runs += [("topk", k, Q, fx[f"{label}__topk{k}__scores_only"]) for k in case.get("topk_only", ())]
    for agg, agg_k, probes, want in runs:
        pre = f"{label}__{agg}{agg_k}"
        if not exact:
            # the cap that keeps the order rule from hiding a failure, asserted from the fixture first
            near = IC.near_pairs(want, 5)
            print(pre, "adjacent pairs of the top 5 closer than MARGIN:", near, "of", 5 * len(want))
            assert near <= (2 if label == "seeded" else 0), pre
        for k in _ks(n_ids):
            host = match_identities_host(probes, E, offsets, agg, agg_k, k) if exact else None
            for path in (FUSED, COMPOSED):
                idx, score = _match(lib, handle, probes, agg, agg_k, k, path)
                if exact:
                    assert np.array_equal(idx, host[0]) and score.tobytes() == host[1].tobytes(), (pre, k, path)
                excused = IC.check_topk(idx, score, want, k, exact=exact)
                drift = np.abs(score - np.take_along_axis(want, idx.astype(np.int64), axis=1)).max()
                print(pre, "k", k, "path", path, "excused positions", excused, "max |score - ref|", drift)
                assert excused <= (0 if exact else 2 * IC.near_pairs(want, k)), (pre, k, path)


# ---------------------------------------------------------------- tile and lane edges
@pytest.fixture(scope="module")
def edge():
    from facerecognitionpipeline_amd.evaluate_models import identity_scores_host, similarity_matrix_host
    Q, E, offsets = IC.edge_case()
    sim = similarity_matrix_host(Q, E)
    ref = {run: identity_scores_host(sim, offsets, *run) for run in IC.EDGE_RUNS}  # computed once, left unchanged
    return Q, E, offsets, ref


def _scatter(idx, score, n_ids):
    """The full score matrix of a k = n_ids result."""
    out = np.empty((len(idx), n_ids), f32)
    np.put_along_axis(out, idx.astype(np.int64), score, axis=1)
    return out


def test_tile_and_lane_edges(lib, handle, edge):
    Q, E, offsets, ref = edge
    n_ids = len(offsets) - 1
    handle.samples_set(_dev(E), offsets)
    excused = compared = 0
    # 10 and 11 queries x 6,184 rows lie on both sides of the built-in rule's 65,536 query-rows
    for n in (1, 3, 10, 11, 16, 17, 40):
        for run in IC.EDGE_RUNS:
            agg, agg_k = run
            got = {}
            for path in (FUSED, COMPOSED, RULE):
                for k in (5, n_ids):
                    idx, score = _match(lib, handle, Q[:n], agg, agg_k, k, path)
                    got[path, k] = (idx, score)
                    if path != RULE:
                        excused += IC.check_topk(idx, score, ref[run][:n], k)  # against match_identities_host
                        compared += idx.size
            # the fused path against the composed one, under the same rule
            excused += IC.check_topk(*got[FUSED, n_ids], _scatter(*got[COMPOSED, n_ids], n_ids), n_ids)
            compared += n * n_ids
            # the built-in rule: one query, or up to 16 with n * rows <= 65,536, take the fused kernel
            took = FUSED if n == 1 or (n <= 16 and n * len(E) <= 65536) else COMPOSED
            for k in (5, n_ids):
                assert np.array_equal(got[RULE, k][0], got[took, k][0]), (n, run, k)
                assert got[RULE, k][1].tobytes() == got[took, k][1].tobytes(), (n, run, k)
    print("excused positions", excused, "of", compared)
    assert excused <= compared // 100


def test_scores_do_not_depend_on_the_tile_cut(lib, handle, edge):
    """An identity's score is a function of its own rows: whichever tile it lands in (caps 64, 128 and
    256 rows and one identity per tile, identities over the cap alone) and whichever queries share the launch."""
    Q, E, offsets, _ref = edge
    n_ids = len(offsets) - 1
    got = {}
    try:
        for cap in (0, 128, 256, 1):
            assert lib.frt_set_identify_tile_rows(cap) == 0
            handle.samples_set(_dev(E), offsets)
            got[cap] = [_match(lib, handle, Q[:3], agg, agg_k, n_ids, FUSED) for agg, agg_k in IC.EDGE_RUNS]
    finally:
        assert lib.frt_set_identify_tile_rows(0) == 0
        handle.samples_set(_dev(E), offsets)
    for cap in (128, 256, 1):
        for (idx, score), (idx0, score0) in zip(got[cap], got[0]):
            assert np.array_equal(idx, idx0) and score.tobytes() == score0.tobytes(), cap
    alone = _match(lib, handle, Q[2:3], "topk", 3, n_ids, FUSED)
    assert np.array_equal(alone[0], got[0][3][0][2:3]) and alone[1].tobytes() == got[0][3][1][2:3].tobytes()


# ---------------------------------------------------------------- embed + match in one call
@pytest.fixture(scope="module")
def embedder():
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    return FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=64)


def test_embed_match_identities(lib, embedder):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops
    from facerecognitionpipeline_amd import weights as W
    h = embedder.model
    rows = embedder.embed_tensor(embedder.to_device_crops(list(W.synthetic_crops(20))), normalize=True)
    offsets = [0, 1, 3, 6, 10, 15, 20]
    h.samples_set(rows.contiguous(), offsets)
    hid = torch_ops.register(embedder)
    try:
        crops = W.probe_crops(W.synthetic_crops(20), 40, sigma=SIGMA, seed=77)
        for n in (1, 5, 40):
            rgb = embedder.to_device_crops(list(crops[:n]))
            for agg, agg_k, k in (("topk", 3, 3), ("max", 3, 6), ("mean", 3, 1)):
                want_emb = torch.empty((n, 512), dtype=torch.float32, device="cuda")
                h.embed(rgb, want_emb, True)
                idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
                score = torch.empty((n, k), dtype=torch.float32, device="cuda")
                emb = torch.empty((n, 512), dtype=torch.float32, device="cuda")
                h.embed_match_identities(rgb, agg, agg_k, k, idx, score, emb)
                assert torch.equal(emb, want_emb), (n, agg)  # bit for bit
                idx2, score2 = torch.empty_like(idx), torch.empty_like(score)
                h.match_identities(emb, agg, agg_k, k, idx2, score2)
                assert torch.equal(idx, idx2) and torch.equal(score, score2), (n, agg)
                idx3, score3 = torch.empty_like(idx), torch.empty_like(score)
                h.embed_match_identities(rgb, agg, agg_k, k, idx3, score3)  # without emb_out
                assert torch.equal(idx, idx3) and torch.equal(score, score3), (n, agg)
                oi, os_, oe = torch.ops.frhip.embed_match_identities(rgb, hid, agg, agg_k, k)
                assert torch.equal(oi, idx) and torch.equal(os_, score) and torch.equal(oe, emb)
                oi, os_ = torch.ops.frhip.match_identities(emb, hid, agg, agg_k, k)
                assert torch.equal(oi, idx) and torch.equal(os_, score)
                if agg == "max":  # probe p is a near-duplicate of crop p mod 20: that row's identity is the best
                    want_id = np.searchsorted(offsets, np.arange(n) % 20, side="right") - 1
                    assert np.array_equal(idx[:, 0].cpu().numpy(), want_id), n
        with FakeTensorMode():
            fi, fs, fe = torch.ops.frhip.embed_match_identities(
                torch.empty(7, 112, 112, 3, dtype=torch.uint8, device="cuda"), hid, "topk", 3, 4)
            assert fi.shape == (7, 4) and fi.dtype == torch.int32 and fi.device.type == "cuda"
            assert fs.shape == (7, 4) and fs.dtype == torch.float32
            assert fe.shape == (7, 512) and fe.dtype == torch.float32
            fi, fs = torch.ops.frhip.match_identities(torch.empty(7, 512, device="cuda"), hid, "max", 3, 2)
            assert fi.shape == (7, 2) and fi.dtype == torch.int32 and fs.shape == (7, 2) and fs.dtype == torch.float32
    finally:
        torch_ops.unregister(hid)
        h.samples_set(torch.empty((0, 512), dtype=torch.float32, device="cuda"), [0])


# ---------------------------------------------------------------- state
def test_sample_gallery_state(lib):
    from facerecognitionpipeline_amd import _lib
    from facerecognitionpipeline_amd.evaluate_models import match_identities_host, pack_gallery
    h = _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=1)
    r = np.random.Generator(np.random.PCG64(0x1DE7_0004))
    unit = lambda *shape: EC._unit(r.standard_normal(shape))  # noqa: E731
    Q = unit(5, 512)
    idx = torch.empty((5, 2), dtype=torch.int32, device="cuda")
    score = torch.empty((5, 2), dtype=torch.float32, device="cuda")
    assert h.samples_size() == (0, 0)
    with pytest.raises(_lib.FrHipError, match="sample gallery is empty"):
        h.match_identities(_dev(Q), "topk", 3, 2, idx, score)
    E1, off1 = unit(9, 512), [0, 2, 3, 9]
    E2, off2 = unit(7, 512), [0, 1, 2, 4, 7]

    def got(k):
        i = torch.empty((5, k), dtype=torch.int32, device="cuda")
        s = torch.empty((5, k), dtype=torch.float32, device="cuda")
        h.match_identities(_dev(Q), "topk", 3, k, i, s)
        return i.cpu().numpy(), s.cpu().numpy()

    def same(a, b):
        return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()

    h.samples_set(torch.from_numpy(E1), off1)  # from host memory
    assert h.samples_size() == (3, 9)
    first = got(3)
    IC.check_topk(*first, _scatter(*match_identities_host(Q, E1, off1, "topk", 3, 3), 3), 3)
    with pytest.raises(ValueError, match="k must be in"):
        got(4)
    with pytest.raises(ValueError):
        got(0)
    with pytest.raises(NotImplementedError, match="agg_k"):
        h.match_identities(_dev(Q), "topk", 17, 2, idx, score)
    with pytest.raises(ValueError):
        h.samples_set(_dev(E1), [0, 2, 3, 8])  # offsets that do not end at the rows
    assert h.samples_size() == (3, 9) and same(got(3), first)
    # a second set replaces the first
    pack_gallery({f"p{i}": {"embeddings": E2[off2[i]:off2[i + 1]]} for i in range(4)}).to_samples(h)
    assert h.samples_size() == (4, 7)
    second = got(4)
    IC.check_topk(*second, _scatter(*match_identities_host(Q, E2, off2, "topk", 3, 4), 4), 4)
    # the template gallery and the sample gallery do not see each other
    T = _dev(unit(6, 512))
    h.gallery_set(T)
    ti, ts = torch.empty((5, 3), dtype=torch.int32, device="cuda"), torch.empty((5, 3), dtype=torch.float32, device="cuda")
    h.match(_dev(Q), 3, ti, ts)
    before = (ti.cpu().numpy(), ts.cpu().numpy())
    assert same(got(4), second)  # after gallery_set + match
    h.samples_set(_dev(E1), off1)
    assert same(got(3), first) and h.gallery_size() == 6
    h.match(_dev(Q), 3, ti, ts)
    assert same((ti.cpu().numpy(), ts.cpu().numpy()), before)  # after the sample calls
    # no identities: cleared
    h.samples_set(torch.empty((0, 512), dtype=torch.float32), [0])
    assert h.samples_size() == (0, 0)
    with pytest.raises(_lib.FrHipError, match="sample gallery is empty"):
        got(1)
    h.match(_dev(Q), 3, ti, ts)
    assert same((ti.cpu().numpy(), ts.cpu().numpy()), before)
    h.close()


# ---------------------------------------------------------------- GalleryManager / FaceMatcher
ROWS_PER_STUDENT = (1, 2, 3, 4, 5, 6, 2, 3)


@pytest.fixture(scope="module")
def matcher(embedder, tmp_path_factory):
    from facerecognitionpipeline_amd import weights as W
    from facerecognitionpipeline_amd.face_matcher import FaceMatcher
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    base = W.synthetic_crops(9)
    gm = GalleryManager(gallery_path=str(tmp_path_factory.mktemp("ident") / "students.npz"), device=embedder.device,
                        verbose=False)
    for i, n in enumerate(ROWS_PER_STUDENT):
        crops = [base[i]] + list(W.probe_crops(base[i:i + 1], n - 1, sigma=SIGMA, seed=100 + i))
        gm.add_student(f"S{i:03d}", f"Student {i}", embedder.extract_embeddings_batch(crops).astype(np.float64))
    fm = FaceMatcher(similarity_threshold=0.5, aggregation_method="consensus", architecture="ir_50", embedder=embedder,
                     gallery=gm, verbose=False, identity_aggregation="topk", identity_k=3)
    return fm, base


def _check_search(gm, q, agg):
    from facerecognitionpipeline_amd.evaluate_models import identify_probe
    got = gm.search_batch(q, 5, aggregation=agg)
    gallery = {sid: {"embeddings": rec.embeddings} for sid, rec in gm.students.items()}
    assert len(got) == len(q)
    for p, res in enumerate(got):
        name, best, scores = identify_probe(q[p], gallery, 0.0, agg, 3)
        assert len(res) == min(5, len(gallery)) and res[0][0] == name, (agg, p)
        assert abs(res[0][2] - float(best)) <= EC.SCORE_TOL
        for sid, sname, s in res:
            assert sname == gm.students[sid].name and abs(s - float(scores[sid])) <= EC.SCORE_TOL, (agg, p, sid)
        assert [s for _i, _n, s in res] == sorted((s for _i, _n, s in res), reverse=True)
    assert gm.search(q[0], 5, aggregation=agg) == got[0]
    return got


def test_gallery_manager_identity_search(matcher, embedder):
    from facerecognitionpipeline_amd import weights as W
    fm, base = matcher
    gm = fm.gallery
    probes = [c for i in (0, 3, 5, 7) for c in W.probe_crops(base[i:i + 1], 2, sigma=SIGMA, seed=200 + i)]
    q = embedder.extract_embeddings_batch(probes)
    template = gm.search_batch(q, 5)  # before any sample upload
    assert [r[0][0] for r in template] == ["S000", "S000", "S003", "S003", "S005", "S005", "S007", "S007"]
    for agg in ("max", "mean", "topk"):
        got = _check_search(gm, q, agg)
        assert [r[0][0] for r in got] == [r[0][0] for r in template]
    assert gm.search_batch(q, 5) == template  # aggregation=None is untouched by the sample upload
    # the sample gallery follows the records
    new = [base[8]] + list(W.probe_crops(base[8:9], 2, sigma=SIGMA, seed=108))
    q8 = embedder.extract_embeddings_batch(list(W.probe_crops(base[8:9], 1, sigma=SIGMA, seed=208)))
    assert gm.search(q8[0], 1, aggregation="topk")[0][0] != "S008"
    gm.add_student("S008", "Student 8", embedder.extract_embeddings_batch(new))
    assert gm.search(q8[0], 1, aggregation="topk")[0][0] == "S008"
    _check_search(gm, np.concatenate([q, q8]), "topk")
    more = embedder.extract_embeddings_batch(list(W.probe_crops(base[0:1], 3, sigma=SIGMA, seed=300)))
    gm.update_embeddings("S000", more, mode="append")
    assert len(gm.students["S000"].embeddings) == 4
    _check_search(gm, np.concatenate([q, q8]), "mean")
    gm.delete_student("S003")
    got = _check_search(gm, np.concatenate([q, q8]), "max")
    assert all(sid != "S003" for res in got for sid, _n, _s in res)
    idx, score = gm.search_identities_device(_dev(q), 2, "max", 3)
    ids = list(gm.students)
    assert [ids[i] for i in idx[:, 0].tolist()] == [r[0][0] for r in got[:len(q)]]
    assert np.abs(score[:, 0].cpu().numpy() - np.array([r[0][2] for r in got[:len(q)]], f32)).max() == 0


def _check_decision(fm, got, frame_match_list):
    agg = fm._aggregate_matches(frame_match_list, {})
    assert got["recognized"] == (agg is not None)
    assert got["frame_matches"] == frame_match_list
    if agg is not None:
        assert (got["student_id"], got["name"], got["confidence"]) == (agg["student_id"], agg["name"],
                                                                       agg["confidence"])
        assert got["method"] == fm.aggregation_method and got["num_frames"] == len(frame_match_list)
    else:
        assert got["reason"] == "below_threshold"
        assert got["best_candidate"] == fm._get_best_candidate(frame_match_list, {})


def test_face_matcher_identity_tracks(matcher):
    from facerecognitionpipeline_amd import weights as W
    from facerecognitionpipeline_amd.evaluate_models import identify_probe
    fm, base = matcher

    def probes(i, n, seed):
        return list(W.probe_crops(base[i:i + 1], n, sigma=SIGMA, seed=seed))

    tracks = [probes(1, 7, 11), probes(5, 9, 12), probes(2, 2, 13) + probes(4, 2, 14),
              list(W.synthetic_crops(8, seed=0xBEEF)), [], probes(6, 3, 15)]
    frames = [f for t in tracks for f in t]
    got = fm.match_tracks(tracks, top_k=3)
    flat = fm.match_faces(frames, top_k=3)  # the same launch composition
    assert len(got) == 6 and got[4] is None
    at = 0
    for t, fr in enumerate(tracks):
        if not fr:
            continue
        want_fm = [{"frame": f"{i:06d}", "student_id": m[0][0], "name": m[0][1], "score": m[0][2],
                    "top_k_matches": [{"student_id": s, "name": n, "score": sc} for s, n, sc in m]}
                   for i, m in enumerate(flat[at:at + len(fr)])]
        at += len(fr)
        assert all(len(m["top_k_matches"]) == 3 for m in want_fm)
        _check_decision(fm, got[t], want_fm)
    who = [g["student_id"] if g["recognized"] else g["best_candidate"]["student_id"] for g in got if g]
    print("recognized", [g["recognized"] for g in got if g], "winners", who)
    assert [who[0], who[1], who[4]] == ["S001", "S005", "S006"] and got[0]["recognized"] and got[1]["recognized"]
    # the scores are identity scores: identify_probe's on the embeddings of the same launch
    emb = fm.embedder.embed_tensor(fm.embedder.to_device_crops(frames), normalize=True).cpu().numpy()
    gallery = {sid: {"embeddings": rec.embeddings} for sid, rec in fm.gallery.students.items()}
    for p in (0, 7, 16, 28):
        name, best, _scores = identify_probe(emb[p], gallery, 0.0, "topk", 3)
        assert flat[p][0][0] == name and abs(flat[p][0][2] - float(best)) <= EC.SCORE_TOL
    assert fm.match_single_face(frames[0], top_k=3) == fm.match_faces(frames[:1], top_k=3)[0]
    # one library call per batch, and the template path when the switch is off
    fm.identity_aggregation = None
    try:
        plain = fm.match_faces(frames[:4], top_k=3)
    finally:
        fm.identity_aggregation = "topk"
    assert [m[0][0] for m in plain] == ["S001"] * 4 and plain != flat[:4]
