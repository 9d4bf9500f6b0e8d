"""CPU-only: the host statement of the track vote (FaceMatcher._aggregate_matches /
_get_best_candidate / _generate_summary) against the reference's own outputs in
tests/golden/track_consensus.npz (tools/make_golden.py track), and fr_track_consensus'
argument errors."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests._track_cases import (confidence_bound, frame_matches, groups, host_matcher, pool_is_quality,
                                track_slices)


def test_host_mirrors_match_the_reference(golden_dir):
    fx = np.load(os.path.join(golden_dir, "track_consensus.npz"))
    seen = set()
    for g in groups(fx):
        fm_ = host_matcher(g["similarity_threshold"])
        for t, (rows, scores) in enumerate(track_slices(g)):
            fm = frame_matches(rows, scores)
            agg = fm_._aggregate_matches(fm, {})
            cand = fm_._get_best_candidate(fm, {})
            label = str(g["labels"][t])
            seen.add(int(g["status"][t]))
            exact = pool_is_quality(scores)
            bound = 0.0 if exact else confidence_bound(scores)
            # _get_best_candidate: winner, its count, its mean score
            assert cand["student_id"] == f"S{int(g['cand_row'][t]):06d}", label
            assert cand["name"] == f"N{int(g['cand_row'][t])}", label
            assert cand["num_quality_frames"] == int(g["cand_num_quality_frames"][t]), label
            assert abs(cand["confidence"] - float(g["cand_confidence"][t])) <= bound, label
            assert set(cand) == {"student_id", "name", "confidence", "num_quality_frames"}
            # _aggregate_matches: the outcome, and every field of a recognized track
            assert (agg is None) == bool(g["agg_none"][t]), label
            if agg is not None:
                assert exact  # a recognized track has >= 3 quality frames
                assert agg["student_id"] == f"S{int(g['row'][t]):06d}" and agg["name"] == f"N{int(g['row'][t])}"
                assert agg["confidence"] == float(g["confidence"][t]), label
                assert agg["consensus_strength"] == float(g["consensus_strength"][t]), label
                assert agg["num_quality_frames"] == int(g["num_quality_frames"][t]), label
                assert agg["total_frames_evaluated"] == int(g["total_frames_evaluated"][t]), label
                assert all(type(agg[k]) is float for k in ("confidence", "consensus_strength"))
    assert seen == {0, 1, 2, 3}  # the fixture reaches every status


def test_host_vote_record_matches_the_fixture_status(golden_dir):
    """track_consensus_host is what the kernel is compared with on the GPU: its status, winner and
    counts on the fixture are the reference's."""
    from facerecognitionpipeline_amd.face_matcher import track_consensus_host
    fx = np.load(os.path.join(golden_dir, "track_consensus.npz"))
    for g in groups(fx):
        for t, (rows, scores) in enumerate(track_slices(g)):
            rec = track_consensus_host(rows.tolist(), scores.tolist(), 0.55, 3, g["similarity_threshold"])
            assert rec[0] == int(g["status"][t]), str(g["labels"][t])
            assert rec[1] == int(g["cand_row"][t]) and rec[2] == int(g["cand_num_quality_frames"][t])
            assert rec[5] == len(rows) and rec[6] == int((scores.astype(np.float64) >= 0.55).sum())
            assert rec[3] == (rec[6] or rec[5])


def test_empty_track_is_the_references_none_and_indexerror():
    fm_ = host_matcher(0.5)
    assert fm_._aggregate_matches([], {}) is None
    with pytest.raises(IndexError):
        fm_._get_best_candidate([], {})


def test_generate_summary_matches_the_reference(golden_dir):
    fx = np.load(os.path.join(golden_dir, "track_consensus.npz"))
    results = json.loads(str(fx["summary_results"]))
    fm_ = host_matcher(0.5, aggregation_method="consensus")
    n_rec = sum(r["recognized"] for r in results)
    for res, rec, want in ((results, n_rec, json.loads(str(fx["summary_ref"]))),
                           ([], 0, json.loads(str(fx["summary_ref_empty"])))):
        got = fm_._generate_summary(res, rec, len(res) - rec)
        assert list(got) == list(want)  # the reference's keys, in its order
        datetime_ok = got.pop("timestamp")
        want.pop("timestamp")
        assert isinstance(datetime_ok, str) and "T" in datetime_ok
        assert json.loads(json.dumps(got)) == want
    fm_.verbose = False
    fm_._print_summary(fm_._generate_summary(results, n_rec, len(results) - n_rec))


def test_track_consensus_argument_errors_without_gpu():
    """The argument checks come before the handle, so they are reported for a NULL handle too."""
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    idx = (ctypes.c_int32 * 8)()
    score = (ctypes.c_float * 8)()
    out_i = (ctypes.c_int32 * 16)()
    out_d = (ctypes.c_double * 4)()

    def call(idx=idx, score=score, k=1, offsets=(0, 3, 8), n_tracks=2, min_frames=3, out_i=out_i, out_d=out_d):
        off = (ctypes.c_int32 * len(offsets))(*offsets) if offsets is not None else None
        rc = lib.fr_track_consensus(None, idx, score, k, off, n_tracks, 0.55, min_frames, 0.5, out_i, out_d, None)
        return rc, lib.fr_last_error(None)

    for kw, text in (({}, b"NULL handle"),
                     ({"idx": None}, b"NULL buffer"), ({"score": None}, b"NULL buffer"),
                     ({"offsets": None}, b"NULL buffer"), ({"out_i": None}, b"NULL buffer"),
                     ({"out_d": None}, b"NULL buffer"), ({"n_tracks": -1}, b"n_tracks"),
                     ({"k": 0}, b"k must be"), ({"min_frames": 0}, b"min_frames"),
                     ({"offsets": (1, 3, 8)}, b"offsets[0]"),
                     ({"offsets": (0, 0, 8)}, b"track 0 has 0"),            # empty track
                     ({"offsets": (0, 3, 2)}, b"track 1 has -1"),           # decreasing offsets
                     ({"offsets": (0, 3, 3 + 1025)}, b"track 1 has 1025")):  # over-long track
        rc, msg = call(**kw)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, kw
        assert text in msg, (kw, msg)
    assert int(out_i[0]) == 0 and float(out_d[0]) == 0.0  # nothing was written


def test_track_consensus_op_shapes_without_gpu():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        idx = torch.empty(9, 3, dtype=torch.int32)
        score = torch.empty(9, 3, dtype=torch.float32)
        ri, rd = torch.ops.frhip.track_consensus(idx, score, [0, 4, 9], 0.55, 3, 0.5)
        assert ri.shape == (2, 8) and ri.dtype == torch.int32
        assert rd.shape == (2, 2) and rd.dtype == torch.float64
    with pytest.raises(ValueError):  # a CPU tensor: there is no CPU fallback
        torch.ops.frhip.track_consensus(torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1), [0, 2], 0.55, 3, 0.5)
