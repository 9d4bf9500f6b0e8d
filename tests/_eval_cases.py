"""Shared by tools/make_golden.py (evaluate), test_evaluate.py and test_gpu_evaluate.py: the inputs
behind tests/golden/evaluate.npz, regenerated from seeds (the file pins them by SHA-256), the column
orders of the recorded tables, and the margins every recorded case has to keep.

A case is ``{"label", "gallery", "positive", "negative", "runs"}``: ``gallery`` / ``positive`` /
``negative`` are the notebook's ``{name: {'embeddings': float32 [rows,512]}}`` dicts (``positive`` may
also hold segments beside 'all'), and ``runs`` lists the (aggregation, k) pairs the reference is
recorded for.

``exact``   gallery rows are basis vectors e_j and a probe is a hand-built list of float32 scores in
            its first G components plus one filler component (index 511) that brings its norm to 1, so
            every cosine is exactly the listed float32 through the reference's real path and through
            a GEMM in any summation order.
``seeded``  13 identities of 1..1024 unit rows around seeded centroids, positive probes built to land
            on true ranks 1, 2-5, 6-10 and above 10, an unenrolled name, two negative sets, two
            segments.
``norms``   probe rows scaled by 0.5 / 0.98 / 0.995 / 1.5 and some gallery rows by 2.0: both sides of
            the 0.01 rule of ``cosine_similarity``.
"""
import hashlib

import numpy as np

f32 = np.float32
# the notebook's list, and thresholds that are float32 values
NOTEBOOK_THRESHOLDS = np.arange(0.2, 0.91, 0.05)
EXACT_THRESHOLDS = np.concatenate([NOTEBOOK_THRESHOLDS, np.array([0.25, 0.5, 0.75, 0.0])])

PROBE_COLUMNS = ("threshold", "rank1_accuracy", "rank5_accuracy", "rank10_accuracy", "mrr", "tar", "far", "frr",
                 "precision", "recall", "f1_score", "tp", "fp", "fn", "n_probes", "avg_correct_score",
                 "avg_incorrect_score")
PROBE_FLOAT_COLUMNS = ("avg_correct_score", "avg_incorrect_score")  # score statistics: within 1e-6
VER_COLUMNS = ("threshold", "tar", "far", "frr", "tp", "fp", "tn", "fn")
IMP_COLUMNS = ("threshold", "rejection_rate", "far", "tn", "fp", "n_impostors", "avg_impostor_score")
IMP_FLOAT_COLUMNS = ("avg_impostor_score",)
VER_EQUAL = ("roc_auc", "eer", "eer_threshold", "tar_at_far_0.001", "tar_at_far_0.01", "tar_at_far_0.1",
             "n_genuine_pairs", "n_impostor_pairs")
VER_FLOAT = ("dprime", "separation", "genuine_mean", "genuine_std", "impostor_mean", "impostor_std")

SCORE_TOL = 1e-6        # two-sided tolerance of a seeded / norms score against the reference
MARGIN = 4e-6           # twice 2 * SCORE_TOL: no decision of the reference may hang on less
F64_DRIFT = 2e-7        # a reference score against its float64 evaluation

SEEDED_ROWS = (1, 1, 2, 3, 4, 5, 8, 40, 63, 64, 65, 257, 1024)
SEEDED_SEED = 0xE7A1_0002
NORMS_SEED = 0xE7A1_0003
EXACT_SEED = 0xE7A1_0001


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_sha(case) -> str:
    """Pins every embedding of a case: gallery, every positive group ('all' and the segments), negatives."""
    parts = [v["embeddings"] for v in case["gallery"].values()]
    for group in case["positive"].values():
        parts.extend(v["embeddings"] for v in group.values())
    parts.extend(v["embeddings"] for v in case["negative"].values())
    return sha(*parts)


def _unit(x):
    x = np.asarray(x, dtype=np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(f32)


# ---------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------
def _probe_from_scores(scores, G):
    """A unit probe whose dot with e_j is scores[j] (float32) for j < G."""
    s = np.asarray(scores, dtype=f32)
    assert s.shape == (G,) and G <= 511
    v = np.zeros(512, f32)
    v[:G] = s
    rest = 1.0 - float(np.sum(s.astype(np.float64) ** 2))
    assert rest > 0.0, "the listed scores leave no room for the filler component"
    v[511] = f32(np.sqrt(rest))
    assert abs(float(np.linalg.norm(v)) - 1.0) < 1e-6
    return v


def _basis_gallery(rows_per_id):
    gallery, at = {}, 0
    for i, n in enumerate(rows_per_id):
        e = np.zeros((n, 512), f32)
        e[np.arange(n), at + np.arange(n)] = 1.0
        gallery[f"id{i:03d}"] = {"embeddings": e}
        at += n
    return gallery, at


def _neighbours(thr):
    c = f32(thr)
    return [np.nextafter(c, f32(-1)), c, np.nextafter(c, f32(2))]


def _one_row_case(n_ids):
    """One-row identities: max and topk k=1.  Probes as (name, scores)."""
    gallery, G = _basis_gallery([1] * n_ids)
    names = list(gallery)
    small = np.array([0.001 * (j % 5) for j in range(n_ids)], f32)  # many equal scores below the ladder
    order = [(7 * j + 3) % n_ids for j in range(n_ids)] if n_ids > 1 else [0]  # a permutation
    assert sorted(order) == list(range(n_ids))
    depth = min(n_ids, 12)
    ladder = small.copy()
    for pos in range(depth):
        ladder[order[pos]] = f32(0.30 - 0.015 * pos)
    probes = []
    for pos in range(depth):  # the true identity at rank pos + 1
        probes.append((names[order[pos]], ladder))
    if n_ids > depth:  # a true identity among the equal small scores: rank by index order
        probes.append((names[order[depth]], ladder))
        probes.append((names[order[n_ids - 1]], ladder))
    if n_ids >= 2:
        lo, hi = sorted(order[:2])
        tie = ladder.copy()
        tie[lo] = tie[hi] = f32(0.30)  # the two best are equal: the lower index is predicted
        probes.append((names[lo], tie))  # the rival comes after the true identity
        probes.append((names[hi], tie))  # the rival comes before it
    if n_ids >= 3:
        a, b = sorted(order[1:3])
        tie = ladder.copy()
        tie[a] = tie[b] = f32(0.30 - 0.015)  # a tie below the best
        probes.append((names[a], tie))
        probes.append((names[b], tie))
    t = order[0]
    for thr in EXACT_THRESHOLDS[:-1]:  # best score at the threshold's float32 and its neighbours
        for v in _neighbours(thr):
            s = small * f32(0.5)
            s[t] = v
            probes.append((names[t], s))
            if n_ids >= 2:  # ... and the true identity is not the best
                probes.append((names[order[1]], s))
    neg = -(np.abs(ladder) * f32(0.5) + f32(0.01))  # every score below 0: identify_probe returns None
    probes.append((names[int(np.argmax(neg))], neg))
    probes.append((names[order[-1]], neg))
    zero = neg.copy()
    zero[t] = f32(0.0)  # a best score of exactly 0 is a prediction
    probes.append((names[t], zero))
    probes.append(("ghost", ladder))  # not enrolled
    probes.append(("ghost", neg))
    s = small.copy()
    s[t] = f32(0.55)
    probes.append(("phantom", s))
    return gallery, G, probes, [("max", 3), ("topk", 1)]


def _multi_row_case():
    """Multi-row identities with dyadic scores (multiples of 1/64): mean and topk k=3 are exact in
    float32 and in float64 alike."""
    rows = [1, 2, 3, 4, 8, 3, 2]
    gallery, G = _basis_gallery(rows)
    names = list(gallery)
    r = np.random.Generator(np.random.PCG64(EXACT_SEED))
    probes = []
    for p in range(24):
        s = (r.integers(-6, 11, size=G) / 64.0).astype(f32)
        if p % 3 == 0:  # identities 2 and 5 (three rows each) get the same values: equal scores
            s[10 + 8:10 + 8 + 3] = s[3:6]
        if p % 4 == 1:
            s[:] = -np.abs(s) - f32(1 / 64)  # all below 0
        name = names[p % len(names)] if p % 8 != 7 else "ghost"
        probes.append((name, s))
    return gallery, G, probes, [("mean", 3), ("topk", 3)]


def _case_from_probes(label, gallery, G, probes, runs):
    positive = {}
    for name, s in probes:
        positive.setdefault(name, []).append(_probe_from_scores(s, G))
    positive = {k: {"embeddings": np.stack(v)} for k, v in positive.items()}
    enrolled = {k: v for k, v in positive.items() if k in gallery}
    ghosts = {k: v for k, v in positive.items() if k not in gallery}
    return {"label": label, "gallery": gallery, "positive": {"all": positive}, "negative": ghosts, "runs": runs,
            "enrolled_only": {"all": enrolled}}


def exact_cases():
    cases = [_case_from_probes(f"exact_n{n}", *_one_row_case(n)) for n in (1, 2, 9, 10, 11, 300)]
    cases.append(_case_from_probes("exact_multi", *_multi_row_case()))
    return cases


# ---------------------------------------------------------------------------------------------
# seeded
# ---------------------------------------------------------------------------------------------
def seeded_case(seed=SEEDED_SEED):
    r = np.random.Generator(np.random.PCG64(seed))
    n_ids = len(SEEDED_ROWS)
    cent = _unit(r.standard_normal((n_ids, 512)))
    names = [f"person_{i:02d}" for i in range(n_ids)]
    gallery = {}
    for i, n in enumerate(SEEDED_ROWS):
        gallery[names[i]] = {"embeddings": _unit(cent[i][None, :] + 0.02 * r.standard_normal((n, 512)))}
    # target ranks of the three probes of every identity: all four buckets (1, 2-5, 6-10, > 10)
    targets = [1, 3, 7, 12, 1, 2, 9, 1, 5, 11, 1, 6, 13]

    def probe(i, rank):
        w = np.zeros(n_ids)
        w[i] = 0.5
        rivals = [j for j in r.permutation(n_ids) if j != i][:rank - 1]
        for q, j in enumerate(rivals):
            w[j] = 0.5 + 0.06 * (q + 1)
        return _unit(w @ cent.astype(np.float64) + 0.012 * r.standard_normal(512))

    positive = {}
    for i in range(n_ids):
        ranks = [targets[(3 * i + m) % len(targets)] for m in range(3)]
        positive[names[i]] = {"embeddings": np.stack([probe(i, k) for k in ranks])}
    positive["visitor"] = {"embeddings": np.stack([
        _unit((0.3 + 0.1 * m) * cent[(5 * m + 2) % n_ids] + 0.03 * r.standard_normal(512)) for m in range(4)])}
    negative = {
        "real": {"embeddings": np.stack([_unit((0.15 + 0.1 * m) * cent[(3 * m) % n_ids] + 0.03 * r.standard_normal(512))
                                         for m in range(7)])},
        "lfw": {"embeddings": np.stack([_unit((0.1 + 0.08 * m) * cent[(4 * m + 1) % n_ids] +
                                              0.03 * r.standard_normal(512)) for m in range(9)])},
    }
    seg_a = {k: positive[k] for k in names[:7] + ["visitor"]}
    seg_b = {k: positive[k] for k in names[7:]}
    return {"label": "seeded", "gallery": gallery, "positive": {"all": positive, "seg_a": seg_a, "seg_b": seg_b},
            "negative": negative, "runs": [("max", 3), ("mean", 3), ("topk", 3)], "topk_only": (1, 2, 16)}


# ---------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------
def norms_case(seed=NORMS_SEED):
    r = np.random.Generator(np.random.PCG64(seed))
    rows = (2, 3, 1, 4, 2)
    cent = _unit(r.standard_normal((len(rows), 512)))
    gallery = {}
    for i, n in enumerate(rows):
        e = _unit(cent[i][None, :] + 0.02 * r.standard_normal((n, 512)))
        if i in (1, 3):
            e[0] *= f32(2.0)  # an off-unit gallery row inside a unit identity
        if i == 4:
            e *= f32(2.0)
        gallery[f"scaled_{i}"] = {"embeddings": e}
    scales = (1.0, 0.5, 0.98, 0.995, 1.5)
    # Genuine and impostor scores are spread over tenths, not clustered: d' = (mean_g - mean_i) / pooled
    # std moves by about (1 + d') / std times a score's rounding (1e-7 for float32 dots of unit rows), so
    # with std near 0.2 and d' near 1 it stays an order of magnitude inside the 1e-6 it is checked to.
    positive = {}
    for i in range(len(rows)):
        p = [_unit((1.0, 0.55, 0.25)[m] * cent[i] + 0.5 * cent[(i + 1 + m) % len(rows)] + 0.015 * r.standard_normal(512))
             * f32(scales[(i + m) % len(scales)]) for m in range(3)]
        positive[f"scaled_{i}"] = {"embeddings": np.stack(p).astype(f32)}
    negative = {"out": {"embeddings": np.stack([
        _unit((0.1 + 0.1 * m) * cent[m % len(rows)] + 0.03 * r.standard_normal(512)) * f32(scales[m % len(scales)])
        for m in range(6)]).astype(f32)}}
    return {"label": "norms", "gallery": gallery, "positive": {"all": positive}, "negative": negative,
            "runs": [("max", 3), ("mean", 3), ("topk", 3)]}


def all_cases():
    return exact_cases() + [seeded_case(), norms_case()]


# ---------------------------------------------------------------------------------------------
# packing and the margins
# ---------------------------------------------------------------------------------------------
def pack(group):
    """{name: {'embeddings'}} -> (names per row, rows [n,512])."""
    names, rows = [], []
    for name, data in group.items():
        names.extend([name] * len(data["embeddings"]))
        rows.append(np.asarray(data["embeddings"], f32).reshape(-1, 512))
    return names, (np.concatenate(rows) if rows else np.zeros((0, 512), f32))


def offsets_of(gallery):
    return np.concatenate([[0], np.cumsum([len(v["embeddings"]) for v in gallery.values()])]).astype(np.int32)


def true_ids(names, gallery):
    index = {n: i for i, n in enumerate(gallery)}
    return np.array([index.get(n, -1) for n in names], np.int32)


def thresholds_of(case):
    return EXACT_THRESHOLDS if case["label"].startswith("exact") else NOTEBOOK_THRESHOLDS


def float64_scores(Q, E, offsets, aggregation, k):
    """The identity scores of the notebook's definition evaluated in float64."""
    Q, E = Q.astype(np.float64), E.astype(np.float64)
    qn, en = np.linalg.norm(Q, axis=1), np.linalg.norm(E, axis=1)
    unit = (np.abs(qn - 1) < 0.01)[:, None] & (np.abs(en - 1) < 0.01)[None, :]
    dots = Q @ E.T
    sim = np.where(unit, dots, dots / (qn[:, None] * en[None, :]))
    out = np.empty((Q.shape[0], len(offsets) - 1))
    for i in range(len(offsets) - 1):
        seg = sim[:, offsets[i]:offsets[i + 1]]
        if aggregation == "max":
            out[:, i] = seg.max(axis=1)
        elif aggregation == "mean":
            out[:, i] = seg.mean(axis=1)
        else:
            out[:, i] = -np.sort(-seg, axis=1)[:, :min(k, seg.shape[1])].mean(axis=1)
    return out


def check_margins(scores, true_id, neg_scores, thresholds, scores64=None, neg_scores64=None):
    """The conditions the builder asserts on the reference's numbers of a seeded / norms run and the
    GPU test asserts again from the file.  scores [n, n_ids] (positive probes), neg_scores [m, n_ids]."""
    scores = np.asarray(scores, np.float64)
    n, n_ids = scores.shape
    thr = np.asarray(thresholds, np.float64)
    srt = np.sort(scores, axis=1)
    best = srt[:, -1]
    if n_ids > 1:
        assert (srt[:, -1] - srt[:, -2]).min() >= MARGIN, "best against second best"
    enrolled = true_id >= 0
    rows = np.arange(n)[enrolled]
    gen = scores[rows, true_id[enrolled]]
    others = scores[rows].copy()
    others[np.arange(len(rows)), true_id[enrolled]] = np.inf
    assert np.abs(others - gen[:, None]).min() >= MARGIN, "true identity against every other"
    nbest = np.asarray(neg_scores, np.float64).max(axis=1)
    imp = np.concatenate([np.where(np.isinf(others), -np.inf, others).max(axis=1), best[~enrolled], nbest])
    imp = imp[np.isfinite(imp)]
    assert np.abs(gen[:, None] - imp[None, :]).min() >= MARGIN, "genuine against impostor"
    for v in (best, gen, nbest):
        assert np.abs(v[:, None] - thr[None, :]).min() >= MARGIN, "a score near a threshold"
    if scores64 is not None:
        assert np.abs(scores - scores64).max() <= F64_DRIFT
        assert np.abs(np.asarray(neg_scores, np.float64) - neg_scores64).max() <= F64_DRIFT


# ---------------------------------------------------------------------------------------------
# the evaluate_* functions against the recorded reference results
# ---------------------------------------------------------------------------------------------
def _rows_table(rows, cols):
    assert all(tuple(r) == tuple(cols) for r in rows), "column order"
    return np.array([[r[c] for c in cols] for r in rows], np.float64)


def _check_table(got_rows, want, cols, float_cols, exact):
    got = _rows_table(got_rows, cols)
    assert got.shape == want.shape
    for c, name in enumerate(cols):
        if name in float_cols and not exact:
            assert np.abs(got[:, c] - want[:, c]).max() <= SCORE_TOL, name
        else:
            assert np.array_equal(got[:, c], want[:, c]), (name, got[:, c], want[:, c])


def _check_verification(ver, fx, pre, exact):
    _check_table(ver["threshold_results"], fx[pre + "ver_table"], VER_COLUMNS, (), exact)
    assert np.array_equal(np.array([ver[k] for k in VER_EQUAL], np.float64), fx[pre + "ver_equal"]), pre
    assert np.abs(np.array([ver[k] for k in VER_FLOAT], np.float64) - fx[pre + "ver_float"]).max() <= SCORE_TOL, pre
    for key, name in (("genuine_scores", "ver_genuine"), ("impostor_scores", "ver_impostor")):
        got = np.array(ver[key], f32)
        if exact:
            assert got.tobytes() == fx[pre + name].tobytes(), (pre, key)
        else:
            assert np.abs(got - fx[pre + name]).max() <= SCORE_TOL, (pre, key)
    assert ver["fpr"][0] == 0 and ver["tpr"][0] == 0 and ver["fpr"][-1] == 1 and ver["tpr"][-1] == 1
    assert len(ver["fpr"]) == len(ver["tpr"]) and np.all(np.diff(ver["fpr"]) >= 0) and np.all(np.diff(ver["tpr"]) >= 0)


def check_evaluate_functions(EM, fx, case, agg, k, **engine):
    """evaluate_{probes,verification,impostors,segmented}_comprehensive of ``EM`` (run with
    ``engine`` = device= / handle= or nothing) against the reference's recorded results: ranks,
    predictions, every table count and count-derived rate, ROC-AUC, EER and TAR@FAR equal; scores and
    score statistics bit for bit on the exact cases and within SCORE_TOL otherwise."""
    label, gallery = case["label"], case["gallery"]
    exact = label.startswith("exact")
    pre = f"{label}__{agg}{k}__"
    thr = thresholds_of(case)
    gnames = list(gallery)
    packed = EM.pack_gallery(gallery, engine["handle"].device if engine.get("handle") is not None else engine.get("device"))
    res = EM.evaluate_probes_comprehensive(packed, case["positive"], thr, aggregation=agg, k=k, **engine)
    assert list(res) == ["threshold_results", "aggregation", "all_predictions", "per_identity"]
    _check_table(res["threshold_results"], fx[pre + "probe_table"], PROBE_COLUMNS, PROBE_FLOAT_COLUMNS, exact)
    preds = res["all_predictions"]
    names, _Q = pack(case["positive"]["all"])
    assert [p["true_identity"] for p in preds] == names
    rec_i, rec_f = fx[pre + "rec_i"], fx[pre + "rec_f"]
    assert [gnames.index(p["predicted_identity"]) if p["predicted_identity"] is not None else -1 for p in preds] == \
        rec_i[:, 0].tolist()
    ranks = [int(round(1 / p["rank_metrics"]["reciprocal_rank"])) if p["rank_metrics"]["reciprocal_rank"] else 0
             for p in preds]
    assert ranks == rec_i[:, 2].tolist()
    for p, r in zip(preds, ranks):
        assert list(p) == ["true_identity", "predicted_identity", "score", "identity_scores", "rank_metrics"]
        assert [p["rank_metrics"][f"rank{c}"] for c in (1, 5, 10)] == [1 <= r <= c for c in (1, 5, 10)]
    scores = np.array([[p["identity_scores"][g] for g in gnames] for p in preds], f32)
    best = np.array([p["score"] for p in preds], f32)
    if exact:
        assert scores.tobytes() == fx[pre + "scores"].tobytes() and best.tobytes() == rec_f[:, 0].tobytes()
    else:
        assert np.abs(scores - fx[pre + "scores"]).max() <= SCORE_TOL
        assert np.abs(best - rec_f[:, 0]).max() <= SCORE_TOL
    pid = res["per_identity"]
    assert list(pid) == fx[pre + "pid_names"].tolist()
    got = np.array([[v["rank1"], v["rank5"], v["rank10"], v["mrr"], v["n_samples"]] for v in pid.values()], np.float64)
    assert np.array_equal(got, fx[pre + "pid_table"])
    gen = np.array([s for v in pid.values() for s in v["genuine_scores"]], f32)
    imp_sum = np.array([np.sum(np.array(v["impostor_scores"], np.float64)) for v in pid.values()])
    assert np.abs(gen - fx[pre + "pid_genuine"]).max() <= (0 if exact else SCORE_TOL)
    assert np.abs(imp_sum - fx[pre + "pid_impostor_sum"]).max() <= (0 if exact else SCORE_TOL * scores.shape[1] * 8)
    lean = EM.evaluate_probes_comprehensive(packed, case["positive"], thr, aggregation=agg, k=k,
                                            keep_identity_scores=False, **engine)
    assert lean["threshold_results"] == res["threshold_results"] and "identity_scores" not in lean["all_predictions"][0]

    rng = np.random.default_rng(7)
    ver = EM.evaluate_verification_comprehensive(packed, case["positive"], case["negative"], thr, aggregation=agg, k=k,
                                                 rng=rng, **engine)
    _check_verification(ver, fx, pre, exact)
    assert ver["genuine_ci"][0] <= ver["genuine_mean"] <= ver["genuine_ci"][1]
    assert abs(EM.compute_dprime(ver["genuine_scores"], ver["impostor_scores"]) - fx[pre + "dprime_fn"]) <= SCORE_TOL

    imp = EM.evaluate_impostors_comprehensive(packed, case["negative"], thr, aggregation=agg, k=k, rng=rng, **engine)
    assert list(imp) == ["threshold_results", "impostor_scores", "impostor_ci", "mean_impostor_score",
                         "std_impostor_score", "aggregation"]
    _check_table(imp["threshold_results"], fx[pre + "imp_table"], IMP_COLUMNS, IMP_FLOAT_COLUMNS, exact)
    assert np.abs(np.array([imp["mean_impostor_score"], imp["std_impostor_score"]]) - fx[pre + "imp_stats"]).max() \
        <= SCORE_TOL

    segments = [s for s in case["positive"] if s != "all"]
    if segments:
        seg = EM.evaluate_segmented_comprehensive(packed, case["positive"], case["negative"], thr, aggregation=agg,
                                                  k=k, rng=rng, **engine)
        assert list(seg) == segments
        for sname, sres in seg.items():
            spre = pre + f"seg_{sname}__"
            _check_table(sres["identification"]["threshold_results"], fx[spre + "probe_table"], PROBE_COLUMNS,
                         PROBE_FLOAT_COLUMNS, exact)
            assert [gnames.index(p["predicted_identity"]) if p["predicted_identity"] is not None else -1
                    for p in sres["identification"]["all_predictions"]] == fx[spre + "predicted"].tolist()
            _check_verification(sres["verification"], fx, spre, exact)
