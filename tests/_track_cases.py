"""Shared by test_track_consensus.py / test_gpu_track_consensus.py: the groups of
tests/golden/track_consensus.npz (tools/make_golden.py track) and the confidence bounds.

Confidence is compared bit for bit where the pool is the quality frames: every addend is then an
f32 in [0.55, 2), a multiple of 2^-24, and the partial sums of <= 1024 of them are exact in
double, so the mean does not depend on the summation order.  Where there is no quality frame the
pool is every frame (any finite f32) and two n-term double summations in different orders, plus
the divisions, stay within n * 2^-52 * max|score|.
"""
from __future__ import annotations

import numpy as np

MIN_QUALITY = 0.55
PER_TRACK = ("labels", "agg_none", "status", "row", "confidence", "consensus_strength", "num_quality_frames",
             "total_frames_evaluated", "cand_row", "cand_confidence", "cand_num_quality_frames")


def groups(fx):
    """One dict per (k, similarity_threshold) group of the fixture: what one launch takes."""
    out = []
    for g in range(int(fx["n_groups"])):
        d = {n: fx[f"g{g}_{n}"] for n in PER_TRACK + ("idx", "score", "offsets")}
        d["k"] = int(fx[f"g{g}_k"])
        d["similarity_threshold"] = float(fx[f"g{g}_similarity_threshold"])
        assert d["idx"].shape == d["score"].shape == (int(d["offsets"][-1]), d["k"])
        assert d["idx"].dtype == np.int32 and d["score"].dtype == np.float32 and np.isfinite(d["score"]).all()
        out.append(d)
    return out


def track_slices(g):
    """(top-1 rows, top-1 f32 scores) of every track of a group."""
    off = g["offsets"]
    return [(g["idx"][a:b, 0], g["score"][a:b, 0]) for a, b in zip(off[:-1], off[1:])]


def frame_matches(rows, scores):
    """The reference's frame_matches entries (face_matcher.py:95-104) for top-1 rows / scores:
    row r is student S<r>, named N<r>; the score is the Python float of the f32."""
    return [{"frame": f"{i:06d}.jpg", "student_id": f"S{int(r):06d}", "name": f"N{int(r)}", "score": float(s)}
            for i, (r, s) in enumerate(zip(rows, scores))]


def pool_is_quality(scores) -> bool:
    return bool((np.asarray(scores, np.float32).astype(np.float64) >= MIN_QUALITY).any())


def confidence_bound(scores) -> float:
    s = np.asarray(scores, np.float64)
    return len(s) * 2.0 ** -52 * float(np.abs(s).max())


def host_matcher(similarity_threshold: float, aggregation_method: str = "majority_vote"):
    """A FaceMatcher without a model or a gallery: the vote and summary functions read only these."""
    from facerecognitionpipeline_amd.face_matcher import FaceMatcher
    fm = FaceMatcher.__new__(FaceMatcher)
    fm.similarity_threshold = similarity_threshold
    fm.aggregation_method = aggregation_method
    fm.verbose = False
    return fm
