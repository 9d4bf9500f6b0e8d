"""Offline model evaluation: the identification / verification functions of the reference's
``evaluate_models_v2.ipynb`` with their names, arguments and result keys, on the GPU.

The notebook scores every identity by the max, mean or top-k mean of a probe's cosines against all
of that identity's gallery embeddings, ranks the identities and sweeps a threshold list, in nested
Python loops over pairs.  Here a probe set is one ``fr_identity_scores`` launch (the score GEMM
against the packed gallery, then a segmented reduction) and one ``fr_eval_probes`` launch (best
identity, rank, genuine / impostor score per probe and the tp / fp / fn counts of every threshold);
the result dicts are built from the records.

``identity_scores_host`` and ``eval_probes_host`` state the two kernels' contracts in numpy, for any
``k`` and any sizes.  The four ``evaluate_*`` functions take ``device=`` or ``handle=``; without
either they run on the host statements (that is how the CPU tests check them against the
reference's recorded results), and ``aggregation='topk'`` with ``k > 16`` always takes the host
statement for the scores.  ``pack_gallery`` packs and uploads a gallery dict once; every function
accepts its result in place of the dict.

``match_identities_host`` states ``fr_match_identities``' contract, the serving counterpart of the
identity scores (the top-k identities of a query against a sample gallery resident in a handle), and
``PackedGallery.to_samples(handle)`` makes an evaluated gallery that sample gallery.

Two deviations from the notebook, both on purpose:

* ``threshold_results`` is a list of row dicts in the reference's column order, not a DataFrame:
  ``pd.DataFrame(rows)`` is the reference's frame, and pandas is not a dependency.
* ``fpr`` / ``tpr`` of the verification result are the full ROC curve at the distinct scores, not
  sklearn's thinned one (``drop_intermediate``); ``roc_auc`` is computed on the thinned curve as
  sklearn does and equals ``sklearn.metrics.auc(*roc_curve(...)[:2])``.

Also: thresholds are compared as float64 (the notebook's are ``np.arange`` elements), the score
statistics (means, standard deviations, d') are float32 like the notebook's,
``bootstrap_confidence_interval`` takes an optional ``rng``, embedding rows
that are not finite or all zero raise ``ValueError``, and the notebook's progress bars and prints are
left out.  Plots, tables and the summary cells are out of scope.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

AGGREGATIONS = ("max", "mean", "topk")
EVAL_MAX_ROWS = 1024       # FR_EVAL_MAX_ROWS
EVAL_MAX_K = 16            # FR_EVAL_MAX_K
EVAL_MAX_THRESHOLDS = 256  # FR_EVAL_MAX_THRESHOLDS
RANKS = (1, 5, 10)
TARGET_FARS = (0.001, 0.01, 0.1)


# ---------------------------------------------------------------------------------------------
# host statements of the kernels' contracts
# ---------------------------------------------------------------------------------------------
def row_norms_host(x: np.ndarray) -> np.ndarray:
    """The row norms ``fr_identity_scores`` applies its 0.01 rule to: the float32 rounding of the
    square root of the float64 sum of squares."""
    x = np.asarray(x, dtype=np.float32)
    return np.sqrt(np.einsum("ij,ij->i", x.astype(np.float64), x.astype(np.float64))).astype(np.float32)


def similarity_matrix_host(Q: np.ndarray, E: np.ndarray) -> np.ndarray:
    """``sim[p][r] = cosine_similarity(Q[p], E[r])`` as ``fr_identity_scores`` defines it: the float32
    dot when both row norms are within 0.01 of 1, else ``dot / (norm_q * norm_e)`` in float32."""
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    E = np.ascontiguousarray(E, dtype=np.float32)
    dots = Q @ E.T
    qn, en = row_norms_host(Q), row_norms_host(E)
    unit = (np.abs(qn - np.float32(1.0)) < np.float32(0.01))[:, None] & \
           (np.abs(en - np.float32(1.0)) < np.float32(0.01))[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = dots / (qn[:, None] * en[None, :])
    return np.where(unit, dots, scaled).astype(np.float32)


def identity_scores_host(sim: np.ndarray, offsets: Sequence[int], aggregation: str = "mean", k: int = 3) -> np.ndarray:
    """What ``fr_identity_scores`` writes to ``out`` for the similarity matrix ``sim`` [n, G]: per
    identity i (columns [offsets[i], offsets[i+1])) the float32 maximum ('max'), the float32 rounding of
    (float64 sum in column order) / count ('mean'), or the ``min(k, count)`` largest values summed in
    float64 in descending order, divided by their number and rounded to float32 ('topk').  Any ``k >= 1``."""
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be one of {list(AGGREGATIONS)}")
    sim = np.asarray(sim, dtype=np.float32)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if sim.ndim != 2 or off.shape[0] < 2 or off[0] != 0 or off[-1] != sim.shape[1] or np.any(np.diff(off) < 1):
        raise ValueError("offsets must start at 0, rise and end at the columns of sim")
    if aggregation == "topk" and k < 1:
        raise ValueError("k must be >= 1")
    out = np.empty((sim.shape[0], off.shape[0] - 1), dtype=np.float32)
    for i in range(off.shape[0] - 1):
        seg = sim[:, off[i]:off[i + 1]]
        if aggregation == "max":
            out[:, i] = seg.max(axis=1)
        elif aggregation == "mean":
            # cumsum adds one column at a time: the fixed order of the kernel's loop
            out[:, i] = (np.cumsum(seg.astype(np.float64), axis=1)[:, -1] / seg.shape[1]).astype(np.float32)
        else:
            m = min(int(k), seg.shape[1])
            top = -np.sort(-seg, axis=1)[:, :m].astype(np.float64)
            out[:, i] = (np.cumsum(top, axis=1)[:, -1] / m).astype(np.float32)
    return out


def match_identities_host(Q: np.ndarray, rows: np.ndarray, offsets: Sequence[int], aggregation: str = "mean",
                          agg_k: int = 3, k: int = 3) -> Tuple[np.ndarray, np.ndarray]:
    """What ``fr_match_identities`` returns for queries ``Q`` [n,512] against the sample gallery
    (``rows`` [G,512], ``offsets``): ``(idx int32 [n,k], score float32 [n,k])``, the ``k`` largest of
    ``identity_scores_host(similarity_matrix_host(Q, rows), offsets, aggregation, agg_k)`` per query in
    descending order, equal scores with the lower identity index first (Python's stable
    ``sorted(..., reverse=True)`` over the dict order in ``identify_probe``).  Any ``agg_k >= 1``."""
    scores = identity_scores_host(similarity_matrix_host(Q, rows), offsets, aggregation, agg_k)
    n, n_ids = scores.shape
    k = int(k)
    if k < 1 or k > n_ids:
        raise ValueError(f"k must be in [1, {n_ids}]")
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]  # stable: equal scores keep the index order
    return order.astype(np.int32), np.take_along_axis(scores, order, axis=1)


def eval_probes_host(scores: np.ndarray, true_id: Sequence[int], thresholds: Sequence[float]
                     ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What ``fr_eval_probes`` computes (include/frhip.h): ``(rec_i int32 [n,4], rec_f float32 [n,4],
    counts int64 [T,4])`` for a score matrix [n, n_ids], the probes' true identity indices (outside
    [0, n_ids): not enrolled) and float64 thresholds (any number of them)."""
    a = np.asarray(scores, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError("expected scores [n, n_ids] with n_ids >= 1")
    n, n_ids = a.shape
    t = np.asarray(true_id, dtype=np.int64).reshape(-1)
    if t.shape[0] != n:
        raise ValueError("true_id must have one entry per probe")
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    rows = np.arange(n)
    best = np.argmax(a, axis=1) if n else np.zeros(0, np.int64)  # first maximum: the lowest index
    bv = a[rows, best]
    predicted = np.where(bv < 0, -1, best)
    enrolled = (t >= 0) & (t < n_ids)
    tc = np.where(enrolled, t, 0)
    at = np.where(enrolled, a[rows, tc], np.float32(0.0)).astype(np.float32)
    j = np.arange(n_ids)[None, :]
    rank = 1 + (a > at[:, None]).sum(axis=1) + ((a == at[:, None]) & (j < tc[:, None])).sum(axis=1)
    rank = np.where(enrolled, rank, 0)
    if n_ids > 1:
        masked = np.where(j == tc[:, None], -np.inf, a)
        others = masked.max(axis=1).astype(np.float32)
    else:
        others = np.full(n, -1.0, np.float32)
    impostor = np.where(enrolled, others, bv).astype(np.float32)
    has_imp = np.where(enrolled, n_ids > 1, True)
    rec_i = np.stack([predicted, best, rank, has_imp.astype(np.int64)], axis=1).astype(np.int32).reshape(n, 4)
    rec_f = np.stack([bv, at, impostor, np.zeros(n, np.float32)], axis=1).astype(np.float32).reshape(n, 4)
    counts = np.zeros((thr.shape[0], 4), dtype=np.int64)
    bv64, at64 = bv.astype(np.float64), at.astype(np.float64)
    correct = enrolled & (predicted == t)
    for q, th in enumerate(thr):
        accepted = bv64 >= th
        tp = accepted & correct
        counts[q] = (tp.sum(), (accepted & ~tp).sum(), (~accepted).sum(), (enrolled & (at64 >= th)).sum())
    return rec_i, rec_f, counts


# ---------------------------------------------------------------------------------------------
# the notebook's small functions
# ---------------------------------------------------------------------------------------------
def cosine_similarity(emb1: np.ndarray, emb2: np.ndarray) -> float:
    """The plain dot of two embeddings whose norms are both within 0.01 of 1, else the dot divided
    by the product of the norms."""
    n1, n2 = np.linalg.norm(emb1), np.linalg.norm(emb2)
    dot = np.dot(emb1, emb2)
    if abs(n1 - 1.0) < 0.01 and abs(n2 - 1.0) < 0.01:
        return dot
    return dot / (n1 * n2)


def compute_all_similarities(probe_emb: np.ndarray, gallery_embeddings) -> List[Tuple[str, float]]:
    """(identity name, cosine) for every gallery embedding, in gallery order."""
    g = pack_gallery(gallery_embeddings)
    if not g.names:
        return []
    sim = similarity_matrix_host(np.asarray(probe_emb, np.float32).reshape(1, -1), g.rows)[0]
    counts = np.diff(g.offsets)
    return [(name, s) for name, c, o in zip(g.names, counts, g.offsets[:-1]) for s in sim[o:o + c]]


def aggregate_max(similarities: List[float]) -> float:
    return max(similarities) if len(similarities) else -1


def aggregate_mean(similarities: List[float]) -> float:
    return np.mean(similarities) if len(similarities) else -1


def aggregate_topk(similarities: List[float], k: int = 3) -> float:
    if not len(similarities):
        return -1
    ordered = sorted(similarities, reverse=True)
    return np.mean(ordered[:min(k, len(ordered))])


def _aggregation(aggregation: str) -> str:
    return aggregation if aggregation in AGGREGATIONS else "max"  # the notebook's else branch


def identify_probe(probe_embedding: np.ndarray, gallery_embeddings, threshold: float, aggregation: str = "mean",
                   k: int = 3) -> Tuple[Optional[str], float, Dict[str, float]]:
    """``(best identity or None below the threshold, best score, {identity: score})`` of one probe
    (host statements; the batched form is ``Handle.identity_scores`` + ``Handle.eval_probes``)."""
    g = pack_gallery(gallery_embeddings)
    if not g.names:
        return None, -1, {}
    q = _check_rows(np.asarray(probe_embedding, np.float32).reshape(1, -1), "probe")
    scores = identity_scores_host(similarity_matrix_host(q, g.rows), g.offsets, _aggregation(aggregation), k)[0]
    identity_scores = dict(zip(g.names, scores))
    best = int(np.argmax(scores))
    if scores[best] < threshold:
        return None, scores[best], identity_scores
    return g.names[best], scores[best], identity_scores


def compute_rank_metrics(identity_scores: Dict[str, float], true_identity: str,
                         ranks: Sequence[int] = RANKS) -> Dict[str, float]:
    """rank-k hits and the reciprocal rank of ``true_identity`` in the scores' descending order
    (equal scores in dict order); 0.0 when it has no score."""
    order = [name for name, _ in sorted(identity_scores.items(), key=lambda kv: kv[1], reverse=True)]
    out = {f"rank{r}": true_identity in order[:r] for r in ranks}
    out["reciprocal_rank"] = 1.0 / (order.index(true_identity) + 1) if true_identity in order else 0.0
    return out


def _rank_metrics_of(rank: int, ranks: Sequence[int] = RANKS) -> Dict[str, float]:
    out = {f"rank{r}": bool(1 <= rank <= r) for r in ranks}
    out["reciprocal_rank"] = 1.0 / rank if rank >= 1 else 0.0
    return out


def compute_dprime(genuine_scores: Sequence[float], impostor_scores: Sequence[float]) -> float:
    """(mean_g - mean_i) / sqrt((std_g^2 + std_i^2) / 2) with population standard deviations."""
    if not len(genuine_scores) or not len(impostor_scores):
        return 0.0
    g, i = np.asarray(genuine_scores), np.asarray(impostor_scores)
    pooled = np.sqrt((g.std() ** 2 + i.std() ** 2) / 2)
    return 0.0 if pooled == 0 else float((g.mean() - i.mean()) / pooled)


def bootstrap_confidence_interval(data: Sequence[float], n_bootstrap: int = 1000, confidence: float = 0.95,
                                  rng=None) -> Tuple[float, float]:
    """Percentile interval of the mean over ``n_bootstrap`` resamples.  ``rng`` (a
    ``np.random.Generator`` or ``RandomState``) makes it repeatable; None draws from numpy's global
    generator as the notebook does."""
    if not len(data):
        return (0.0, 0.0)
    data = np.asarray(data)
    choice = np.random.choice if rng is None else rng.choice
    means = [np.mean(choice(data, size=len(data), replace=True)) for _ in range(n_bootstrap)]
    alpha = 1 - confidence
    return (np.percentile(means, alpha / 2 * 100), np.percentile(means, (1 - alpha / 2) * 100))


# ---------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------
def _check_rows(x: np.ndarray, what: str) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != 512:
        raise ValueError(f"{what}: expected embeddings of shape [rows, 512], got {list(x.shape)}")
    if not np.isfinite(x).all():
        raise ValueError(f"{what}: embedding rows must be finite")
    if x.shape[0] and not np.abs(x).max(axis=1).all():
        raise ValueError(f"{what}: an embedding row is all zero")
    return x


class PackedGallery:
    """A gallery dict packed for ``fr_identity_scores``: identity i (``names[i]``) owns rows
    [offsets[i], offsets[i+1]) of ``rows`` float32 [G,512]; ``rows_on(device)`` is its device copy,
    uploaded once."""

    def __init__(self, names: List[str], offsets: np.ndarray, rows: np.ndarray, device=None):
        self.names, self.offsets, self.rows = names, offsets, rows
        self.index = {name: i for i, name in enumerate(names)}
        self._dev = {}
        if device is not None:
            self.rows_on(device)

    def __contains__(self, name) -> bool:
        return name in self.index

    def __len__(self) -> int:
        return len(self.names)

    def rows_on(self, device):
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.rows).to(device)
        return self._dev[device]

    def to_samples(self, handle, tag=None) -> None:
        """Make this gallery the sample gallery of ``handle`` (``Handle.samples_set``): what an
        evaluation scored is then what ``match_identities`` serves, identity i being ``names[i]``."""
        handle.samples_set(self.rows_on(handle.device), self.offsets, tag)


def pack_gallery(gallery_embeddings, device=None) -> PackedGallery:
    """``{name: {'embeddings': array [rows,512]}}`` -> ``PackedGallery`` (returned as is when it
    already is one); with ``device`` the rows are uploaded now.  Identities keep the dict's order."""
    if isinstance(gallery_embeddings, PackedGallery):
        if device is not None:
            gallery_embeddings.rows_on(device)
        return gallery_embeddings
    names, blocks = [], []
    for name, data in gallery_embeddings.items():
        e = _check_rows(np.asarray(data["embeddings"], dtype=np.float32).reshape(-1, 512), f"gallery identity {name!r}")
        if e.shape[0] < 1:
            raise ValueError(f"gallery identity {name!r} has no embeddings")
        names.append(name)
        blocks.append(e)
    offsets = np.zeros(len(names) + 1, dtype=np.int32)
    if names:
        offsets[1:] = np.cumsum([b.shape[0] for b in blocks])
    rows = np.concatenate(blocks, axis=0) if blocks else np.zeros((0, 512), np.float32)
    return PackedGallery(names, offsets, np.ascontiguousarray(rows), device)


def _pack_probes(probe_data, gallery: Optional[PackedGallery]) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """``{name: {'embeddings': array}}`` -> (the name of every probe, true identity index or -1,
    embeddings [n,512]) in dict order.  gallery None: every probe is an impostor (-1)."""
    names, blocks = [], []
    for name, data in probe_data.items():
        e = _check_rows(np.asarray(data["embeddings"], dtype=np.float32).reshape(-1, 512), f"probe set {name!r}")
        names.extend([name] * e.shape[0])
        blocks.append(e)
    Q = np.concatenate(blocks, axis=0) if blocks else np.zeros((0, 512), np.float32)
    true_id = np.array([gallery.index.get(nm, -1) if gallery is not None else -1 for nm in names], dtype=np.int32)
    return names, true_id, np.ascontiguousarray(Q)


def _resolve_handle(device, handle):
    if handle is not None:
        return handle
    if device is None:
        return None
    from .torch_ops import utility_handle
    return utility_handle(device)


class _Scored:
    """One probe set scored against one gallery: the records, the threshold counts and (on request)
    the score matrix on the host."""

    def __init__(self, gallery: PackedGallery, names, true_id, Q, thresholds, aggregation, k, handle):
        self.gallery, self.names, self.true_id = gallery, names, true_id
        thr = np.asarray(list(thresholds), dtype=np.float64).reshape(-1)
        agg = _aggregation(aggregation)
        if len(gallery) < 1:
            raise ValueError("the gallery has no identities")
        if handle is not None and np.diff(gallery.offsets).max() > EVAL_MAX_ROWS:
            raise NotImplementedError(f"an identity has more than {EVAL_MAX_ROWS} gallery rows: evaluate it without "
                                      "device= / handle= (the host statements)")
        host_scores = handle is None or (agg == "topk" and k > EVAL_MAX_K)
        self._scores_host = self._scores_dev = None
        if host_scores:
            self._scores_host = identity_scores_host(similarity_matrix_host(Q, gallery.rows), gallery.offsets, agg, k)
        if handle is None:
            self.rec_i, self.rec_f, self.counts = eval_probes_host(self._scores_host, true_id, thr)
            return
        import torch
        dev = handle.device
        if host_scores:
            self._scores_dev = torch.from_numpy(self._scores_host).to(dev)
        else:
            self._scores_dev = handle.identity_scores(torch.from_numpy(Q).to(dev), gallery.rows_on(dev),
                                                      gallery.offsets, agg, k)
        t_dev = torch.from_numpy(true_id).to(dev)
        counts = []
        for c0 in range(0, max(thr.shape[0], 1), EVAL_MAX_THRESHOLDS):  # one launch for up to 256 thresholds
            rec_i, rec_f, cnt = handle.eval_probes(self._scores_dev, t_dev, thr[c0:c0 + EVAL_MAX_THRESHOLDS])
            counts.append(cnt.cpu().numpy())
        self.rec_i, self.rec_f = rec_i.cpu().numpy(), rec_f.cpu().numpy()
        self.counts = np.concatenate(counts, axis=0)

    @property
    def scores(self) -> np.ndarray:
        if self._scores_host is None:
            self._scores_host = self._scores_dev.cpu().numpy()
        return self._scores_host


def _score(gallery, probe_data, enrolled: bool, thresholds, aggregation, k, handle) -> _Scored:
    names, true_id, Q = _pack_probes(probe_data, gallery if enrolled else None)
    return _Scored(gallery, names, true_id, Q, thresholds, aggregation, k, handle)


# ---------------------------------------------------------------------------------------------
# host-side metrics
# ---------------------------------------------------------------------------------------------
def roc_curve_auc(genuine_scores: np.ndarray, impostor_scores: np.ndarray) -> Tuple[np.ndarray, np.ndarray, float]:
    """(fpr, tpr, auc) of genuine (label 1) against impostor (label 0) scores: the full curve at the
    distinct scores from (0, 0), and the trapezoid area of the curve without its collinear points,
    the value of ``sklearn.metrics.auc(*roc_curve(y_true, y_scores)[:2])``."""
    y_true = np.r_[np.ones(len(genuine_scores)), np.zeros(len(impostor_scores))]
    y_score = np.r_[np.asarray(genuine_scores, np.float32), np.asarray(impostor_scores, np.float32)]
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    idx = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true)[idx]
    fps = 1 + idx - tps
    keep = np.arange(len(fps))
    if len(fps) > 2:  # points on a straight segment change no trapezoid sum but its rounding
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
    fpr, tpr = np.r_[0, fps] / fps[-1], np.r_[0, tps] / tps[-1]
    x, y = np.r_[0, fps[keep]] / fps[-1], np.r_[0, tps[keep]] / tps[-1]
    area = float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())
    return fpr, tpr, area


def _first_min(values: Sequence[float]) -> int:
    return int(np.argmin(np.asarray(values, dtype=np.float64)))  # the first minimum, as Series.idxmin


def _eer_and_tar(rows: List[dict]) -> dict:
    far = np.array([r["far"] for r in rows], dtype=np.float64)
    frr = np.array([r["frr"] for r in rows], dtype=np.float64)
    i = _first_min(np.abs(far - frr))
    out = {"eer": (rows[i]["far"] + rows[i]["frr"]) / 2, "eer_threshold": rows[i]["threshold"]}
    for target in TARGET_FARS:
        out[f"tar_at_far_{target}"] = rows[_first_min(np.abs(far - target))]["tar"]
    return out


def _mean(x):
    return np.mean(x) if len(x) else 0  # float32, as the notebook's np.mean of a list of float32 scores


# ---------------------------------------------------------------------------------------------
# the notebook's evaluate_* functions
# ---------------------------------------------------------------------------------------------
def _probe_dict(probes):
    return probes.get("all", probes)


def _identification(s: _Scored, thresholds, aggregation: str, keep_identity_scores: bool) -> Dict:
    names, gnames = s.names, s.gallery.names
    n = len(names)
    rank = s.rec_i[:, 2]
    bv = s.rec_f[:, 0]
    predicted = [gnames[p] if p >= 0 else None for p in s.rec_i[:, 0]]
    metrics = [_rank_metrics_of(int(r)) for r in rank]
    scores = s.scores if keep_identity_scores else None
    all_predictions, per = [], {}
    for p in range(n):
        pred = {"true_identity": names[p], "predicted_identity": predicted[p], "score": bv[p]}
        if scores is not None:
            pred["identity_scores"] = dict(zip(gnames, scores[p]))
        pred["rank_metrics"] = metrics[p]
        all_predictions.append(pred)
        pid = per.setdefault(names[p], {"rank1_total": 0, "rank5_total": 0, "rank10_total": 0, "mrr_sum": 0,
                                        "count": 0, "genuine_scores": [], "impostor_scores": []})
        for r in RANKS:
            pid[f"rank{r}_total"] += 1 if metrics[p][f"rank{r}"] else 0
        pid["mrr_sum"] += metrics[p]["reciprocal_rank"]
        pid["count"] += 1
        pid["genuine_scores"].append(s.rec_f[p, 1] if rank[p] > 0 else 0)
        if scores is not None:
            t = int(s.true_id[p])
            pid["impostor_scores"].extend(np.delete(scores[p], t) if rank[p] > 0 else scores[p])
    hits = {r: int(((rank >= 1) & (rank <= r)).sum()) for r in RANKS}
    mrr_sum = 0
    for m in metrics:
        mrr_sum += m["reciprocal_rank"]
    correct = np.array([predicted[p] == names[p] for p in range(n)], dtype=bool)
    bv64 = bv.astype(np.float64)
    rows = []
    for q, threshold in enumerate(thresholds):
        tp, fp, fn = (int(v) for v in s.counts[q, :3])
        accepted = bv64 >= np.float64(threshold)
        precision = tp / (tp + fp) if (tp + fp) > 0 else 0
        recall = tp / (tp + fn) if (tp + fn) > 0 else 0
        rows.append({
            "threshold": threshold,
            "rank1_accuracy": hits[1] / n if n > 0 else 0,
            "rank5_accuracy": hits[5] / n if n > 0 else 0,
            "rank10_accuracy": hits[10] / n if n > 0 else 0,
            "mrr": mrr_sum / n if n > 0 else 0,
            "tar": tp / n if n > 0 else 0,
            "far": fp / n if n > 0 else 0,
            "frr": fn / n if n > 0 else 0,
            "precision": precision,
            "recall": recall,
            "f1_score": 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0,
            "tp": tp,
            "fp": fp,
            "fn": fn,
            "n_probes": n,
            "avg_correct_score": _mean(bv[accepted & correct]),
            "avg_incorrect_score": _mean(bv[accepted & ~correct]),
        })
    per_identity = {}
    for identity, st in per.items():
        c = st["count"]
        per_identity[identity] = {"rank1": st["rank1_total"] / c, "rank5": st["rank5_total"] / c,
                                  "rank10": st["rank10_total"] / c, "mrr": st["mrr_sum"] / c, "n_samples": c,
                                  "genuine_scores": st["genuine_scores"]}
        if scores is not None:
            per_identity[identity]["impostor_scores"] = st["impostor_scores"]
    return {"threshold_results": rows, "aggregation": aggregation, "all_predictions": all_predictions,
            "per_identity": per_identity}


def evaluate_probes_comprehensive(gallery_embeddings, probe_embeddings, thresholds, aggregation: str = "mean",
                                  k: int = 3, device=None, handle=None, keep_identity_scores: bool = True) -> Dict:
    """Closed- and open-set identification of every probe: ``threshold_results`` (rank-1/5/10
    accuracy, MRR, TAR / FAR / FRR, precision, recall, F1, tp / fp / fn per threshold),
    ``all_predictions`` and the ``per_identity`` table.  ``keep_identity_scores=False`` leaves the
    ``identity_scores`` dicts and the per-identity ``impostor_scores`` lists out, and the score matrix
    on the device."""
    thresholds = list(thresholds)
    h = _resolve_handle(device, handle)
    g = pack_gallery(gallery_embeddings, h.device if h is not None else None)
    s = _score(g, _probe_dict(probe_embeddings), True, thresholds, aggregation, k, h)
    return _identification(s, thresholds, aggregation, keep_identity_scores)


def _verification(pos: _Scored, neg: _Scored, thresholds, aggregation: str, rng) -> Dict:
    enrolled = pos.rec_i[:, 2] > 0
    genuine = pos.rec_f[enrolled, 1]
    impostor = neg.rec_f[:, 0]
    if not len(genuine):
        raise ValueError("No genuine scores collected! Check probe_positive data.")
    if not len(impostor):
        raise ValueError("No impostor scores collected! Check probe_negative data.")
    n_g, n_i = len(genuine), len(impostor)
    rows = []
    for q, threshold in enumerate(thresholds):
        tp = int(pos.counts[q, 3])
        tn = int(neg.counts[q, 2])
        fn, fp = n_g - tp, n_i - tn
        rows.append({"threshold": threshold, "tar": tp / n_g, "far": fp / n_i, "frr": fn / n_g, "tp": tp, "fp": fp,
                     "tn": tn, "fn": fn})
    fpr, tpr, roc_auc = roc_curve_auc(genuine, impostor)
    # float32 statistics of the float32 scores, in the notebook's order of operations
    g_mean, i_mean = np.mean(genuine), np.mean(impostor)
    g_std = np.std(genuine, ddof=1) if n_g > 1 else np.float32("nan")
    i_std = np.std(impostor, ddof=1) if n_i > 1 else np.float32("nan")
    pooled_std = np.sqrt((g_std ** 2 + i_std ** 2) / 2)
    dprime = (g_mean - i_mean) / pooled_std if pooled_std > 0 else 0
    pooled_variance = (g_std ** 2 + i_std ** 2) / 2
    separation = abs(g_mean - i_mean) / np.sqrt(pooled_variance) if pooled_variance > 0 else 0
    return {"threshold_results": rows, "roc_auc": roc_auc, "dprime": dprime, "separation": separation,
            **_eer_and_tar(rows),
            "genuine_mean": g_mean, "genuine_std": g_std, "impostor_mean": i_mean, "impostor_std": i_std,
            "genuine_scores": list(genuine), "impostor_scores": list(impostor),
            "genuine_ci": bootstrap_confidence_interval(genuine, rng=rng),
            "impostor_ci": bootstrap_confidence_interval(impostor, rng=rng),
            "fpr": fpr, "tpr": tpr, "aggregation": aggregation, "n_genuine_pairs": n_g, "n_impostor_pairs": n_i}


def evaluate_verification_comprehensive(gallery_embeddings, probe_positive, probe_negative, thresholds,
                                        aggregation: str = "mean", k: int = 3, device=None, handle=None,
                                        rng=None) -> Dict:
    """Verification: every enrolled positive probe against its own identity (genuine) and every
    negative probe's best identity score (impostor): TAR / FAR / FRR per threshold, ROC-AUC, d',
    separation, EER, TAR@FAR and the score statistics."""
    thresholds = list(thresholds)
    h = _resolve_handle(device, handle)
    g = pack_gallery(gallery_embeddings, h.device if h is not None else None)
    pos = _score(g, _probe_dict(probe_positive), True, thresholds, aggregation, k, h)
    neg_data = _probe_dict(probe_negative) if probe_negative else {}
    neg = _score(g, neg_data, False, thresholds, aggregation, k, h)
    return _verification(pos, neg, thresholds, aggregation, rng)


def evaluate_impostors_comprehensive(gallery_embeddings, impostor_embeddings, thresholds, aggregation: str = "mean",
                                     k: int = 3, device=None, handle=None, rng=None) -> Dict:
    """Open-set rejection: the best identity score of every impostor embedding against the
    threshold list."""
    thresholds = list(thresholds)
    h = _resolve_handle(device, handle)
    g = pack_gallery(gallery_embeddings, h.device if h is not None else None)
    s = _score(g, impostor_embeddings, False, thresholds, aggregation, k, h)
    scores = s.rec_f[:, 0]
    n = len(scores)
    avg = np.mean(scores) if n else np.float32("nan")
    rows = []
    for q, threshold in enumerate(thresholds):
        tn = int(s.counts[q, 2])
        fp = n - tn
        rows.append({"threshold": threshold, "rejection_rate": tn / n if n > 0 else 0, "far": fp / n if n > 0 else 0,
                     "tn": tn, "fp": fp, "n_impostors": n, "avg_impostor_score": avg})
    return {"threshold_results": rows, "impostor_scores": list(scores),
            "impostor_ci": bootstrap_confidence_interval(scores, rng=rng), "mean_impostor_score": avg,
            "std_impostor_score": np.std(scores) if n else np.float32("nan"),
            "aggregation": aggregation}


def evaluate_segmented_comprehensive(gallery_embeddings, probe_positive, probe_negative, thresholds,
                                     aggregation: str = "mean", k: int = 3, include_verification: bool = True,
                                     device=None, handle=None, rng=None, keep_identity_scores: bool = True
                                     ) -> Dict[str, Dict]:
    """``{segment: {'identification': ..., 'verification': ... or None}}`` for every key of
    ``probe_positive`` but 'all'.  The gallery is packed and uploaded once and the negative probes are
    scored once for all segments."""
    thresholds = list(thresholds)
    h = _resolve_handle(device, handle)
    g = pack_gallery(gallery_embeddings, h.device if h is not None else None)
    neg = None
    if include_verification and probe_negative is not None:
        neg = _score(g, _probe_dict(probe_negative) if probe_negative else {}, False, thresholds, aggregation, k, h)
    out = {}
    for segment in [key for key in probe_positive.keys() if key != "all"]:
        pos = _score(g, probe_positive[segment], True, thresholds, aggregation, k, h)
        ver = None
        if neg is not None:
            try:
                ver = _verification(pos, neg, thresholds, aggregation, rng)
            except Exception as e:  # the notebook reports and carries on
                print(f"  Warning: Verification failed for {segment}: {e}")
        out[segment] = {"identification": _identification(pos, thresholds, aggregation, keep_identity_scores),
                        "verification": ver}
    return out


# ---------------------------------------------------------------------------------------------
# reading EmbeddingGenerator's files back (the notebook's load_embeddings / load_all_embeddings)
# ---------------------------------------------------------------------------------------------
EMBEDDING_FILES = {
    "gallery_oneshot_base": "gallery_one-shot_base.pkl",
    "gallery_oneshot_augmented": "gallery_one-shot_augmented.pkl",
    "gallery_fewshot_base": "gallery_few-shot_base.pkl",
    "gallery_fewshot_augmented": "gallery_few-shot_augmented.pkl",
    "probe_positive_unsegmented": "probe_positive_unsegmented.pkl",
    "probe_positive_segmented": "probe_positive_segmented.pkl",
    "probe_negative": "probe_negative.pkl",
}


def load_embedding_pickle(path):
    """``pickle.load`` of one of ``EmbeddingGenerator``'s files -- dicts, lists, str, int, bool and
    numpy arrays -- through the gallery's whitelist unpickler cut down to numpy's reconstruction
    globals: a pickle that names anything else raises ``pickle.UnpicklingError`` and runs nothing."""
    import pickle
    from .gallery_manager import _NUMPY_GLOBALS, _GalleryUnpickler

    class _EmbeddingUnpickler(_GalleryUnpickler):
        def find_class(self, module, name):
            if (module, name) not in _NUMPY_GLOBALS:
                raise pickle.UnpicklingError(f"embedding pickle names a global outside the whitelist: {module}.{name}")
            return super().find_class(module, name)

    with open(path, "rb") as f:
        return _EmbeddingUnpickler(f).load()


def load_embeddings(model_name: str, embeddings_root) -> Dict:
    """The notebook's ``load_embeddings`` (``embeddings_root`` is a global there): the seven files of
    ``<embeddings_root>/<model_name>`` under the notebook's keys, ``None`` for a file that is missing;
    ``FileNotFoundError`` when the model directory is."""
    from pathlib import Path
    model_dir = Path(embeddings_root) / model_name
    if not model_dir.exists():
        raise FileNotFoundError(f"Model directory not found: {model_dir}")
    return {key: load_embedding_pickle(model_dir / filename) if (model_dir / filename).exists() else None
            for key, filename in EMBEDDING_FILES.items()}


def load_all_embeddings(base_dir) -> Dict[str, Dict]:
    """The notebook's ``load_all_embeddings``: every sub-directory of ``base_dir`` is a model, every
    known ``.pkl`` in it a key; an unknown ``.pkl`` is warned about and skipped, a missing one has no key."""
    from pathlib import Path
    mapping = {filename: key for key, filename in EMBEDDING_FILES.items()}
    all_embeddings: Dict[str, Dict] = {}
    for model_dir in sorted(Path(base_dir).iterdir()):
        if not model_dir.is_dir():
            continue
        all_embeddings[model_dir.name] = {}
        for file in sorted(model_dir.iterdir()):
            if file.suffix != ".pkl":
                continue
            key = mapping.get(file.name)
            if key is None:
                print(f"Warning: Unrecognized file {file.name}, skipping…")
                continue
            all_embeddings[model_dir.name][key] = load_embedding_pickle(file)
    return all_embeddings
