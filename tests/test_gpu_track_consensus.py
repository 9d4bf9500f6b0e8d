"""GPU: ``fr_track_consensus`` against the reference's outputs (tests/golden/track_consensus.npz) and
against the host statement of the vote on a seeded batch; its torch op; ``FaceMatcher.match_tracks`` /
``process_capture_directory`` end to end on synthetic weights.  Bounds: tests/_track_cases.py."""
import json
import os

import numpy as np
import pytest
import torch

from tests._track_cases import confidence_bound, groups, pool_is_quality, track_slices

pytestmark = pytest.mark.gpu

# Probe noise of the end-to-end tracks (weights.probe_crops' default).  With the synthetic IR-50 weights
# the CPU oracle (oracle/adaface_net.py) scores every sigma-12 probe of _tracks() >= 0.9993 against its own
# gallery row, >= 0.035 above any other row, and the unrelated crops 0.96 .. 0.965 against every row with
# their top-1 spread over 6 rows (at most 2 of 8 on one): the one-identity tracks are recognized with all
# votes on one row, the 2 + 2 track and the track of unrelated crops have no consensus, and every frame
# is a quality frame (>= 0.55).
SIGMA = 12.0


@pytest.fixture(scope="module")
def handle():
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=1)  # never finalised


def _launch(handle, idx, score, offsets, thr, **kw):
    ri, rd = handle.track_consensus(torch.from_numpy(idx).cuda(), torch.from_numpy(score).cuda(), offsets,
                                    similarity_threshold=thr, **kw)
    assert ri.dtype == torch.int32 and rd.dtype == torch.float64 and ri.is_cuda and rd.is_cuda
    return ri.cpu().numpy(), rd.cpu().numpy()


def test_track_consensus_matches_the_reference(handle, golden_dir):
    fx = np.load(os.path.join(golden_dir, "track_consensus.npz"))
    for g in groups(fx):
        ri, rd = _launch(handle, g["idx"], g["score"], g["offsets"], g["similarity_threshold"])
        assert ri.shape == (len(g["labels"]), 8) and rd.shape == (len(g["labels"]), 2)
        for t, (rows, scores) in enumerate(track_slices(g)):
            label = str(g["labels"][t])
            status, row, count, pool, second, n, nq, pad = (int(v) for v in ri[t])
            conf, ratio = (float(v) for v in rd[t])
            print(label, ri[t].tolist(), repr(conf), repr(ratio), "want", int(g["status"][t]),
                  repr(float(g["cand_confidence"][t])))
            exact = pool_is_quality(scores)
            assert status == int(g["status"][t]), label
            assert (status == 0) == (not g["agg_none"][t]), label
            assert row == int(g["cand_row"][t]) and count == int(g["cand_num_quality_frames"][t]), label
            assert n == len(rows) and nq == int((scores.astype(np.float64) >= 0.55).sum()) and pad == 0, label
            assert pool == (nq or n) and 0 <= second <= count and count + second <= pool, label
            assert ratio == count / pool, label
            if exact:
                assert conf == float(g["cand_confidence"][t]), label
            else:
                assert abs(conf - float(g["cand_confidence"][t])) <= confidence_bound(scores), label
            if status == 0:
                assert row == int(g["row"][t]) and count == int(g["num_quality_frames"][t]), label
                assert conf == float(g["confidence"][t]) and ratio == float(g["consensus_strength"][t]), label
                assert n == int(g["total_frames_evaluated"][t]), label


def _random_batch():
    """200 + 5 tracks: lengths 1..40 and 1 / 255 / 256 / 257 / 1024, rows of 4 ids (ties are common),
    scores of a small f32 grid straddling 0.55; k = 2 with decoys in column 1."""
    r = np.random.Generator(np.random.PCG64(0x7AC5))
    lengths = r.integers(1, 41, size=200).tolist() + [1, 255, 256, 257, 1024]
    ids = np.array([3, 99999, 17, 40000], np.int32)
    grid = np.array([0.30, 0.45, 0.52, 0.54999995, 0.55, 0.58, 0.61, 0.70], np.float32)
    idx, score = [], []
    for t, n in enumerate(lengths):
        # per-track id weights, so that majorities, near ties and scattered votes all occur
        p = r.dirichlet([0.6] * 4)
        # per-track score range: tracks with no (grid[:4] is below 0.55), few and only quality frames
        lo, hi = ((0, 8), (1, 8), (2, 8), (3, 8), (4, 8), (0, 4))[r.integers(0, 6)]
        idx.append(r.choice(ids, size=n, p=p))
        score.append(grid[r.integers(lo, hi, size=n)])
    idx, score = np.concatenate(idx).astype(np.int32), np.concatenate(score).astype(np.float32)
    idx = np.stack([idx, (idx + 1) % 100000], axis=1)
    score = np.stack([score, score * np.float32(0.9)], axis=1)
    return idx, score, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def test_track_consensus_random_batch_equals_host_mirror(handle):
    from facerecognitionpipeline_amd.face_matcher import track_consensus_host
    idx, score, offsets = _random_batch()
    thr = 0.6  # above the grid's lowest quality scores, so BELOW_THRESHOLD occurs
    ri, rd = _launch(handle, idx, score, offsets, thr)
    seen = set()
    for t, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        rows, scores = idx[a:b, 0], score[a:b, 0]
        want = track_consensus_host(rows.tolist(), scores.tolist(), 0.55, 3, thr)
        seen.add(want[0])
        assert ri[t].tolist() == [int(v) for v in want[:7]] + [0], (t, ri[t].tolist(), want)
        assert float(rd[t, 1]) == want[8], (t, rd[t], want)
        bound = 0.0 if pool_is_quality(scores) else confidence_bound(scores)
        assert abs(float(rd[t, 0]) - want[7]) <= bound, (t, repr(float(rd[t, 0])), repr(want[7]))
    assert seen == {0, 1, 2, 3}  # a broken generator cannot hide a branch
    # deterministic, and independent of the launch shape: a track alone gives the record it gives in the batch
    ri2, rd2 = _launch(handle, idx, score, offsets, thr)
    assert np.array_equal(ri, ri2) and np.array_equal(rd, rd2)
    for t in (0, 17, 201, 204):
        a, b = int(offsets[t]), int(offsets[t + 1])
        r1, d1 = _launch(handle, idx[a:b].copy(), score[a:b].copy(), [0, b - a], thr)
        assert np.array_equal(r1[0], ri[t]) and np.array_equal(d1[0], rd[t])


def test_track_consensus_thresholds_are_arguments(handle):
    idx = np.array([[5], [5], [9], [5]], np.int32)
    score = np.array([[0.9], [0.8], [0.7], [0.3]], np.float32)
    ri, rd = _launch(handle, idx, score, [0, 4], 0.5)
    assert ri[0].tolist() == [0, 5, 2, 3, 1, 4, 3, 0] and float(rd[0, 0]) == (float(score[0, 0]) + float(score[1, 0])) / 2
    assert _launch(handle, idx, score, [0, 4], 0.5, min_frames=4)[0][0, 0] == 1
    ri, rd = _launch(handle, idx, score, [0, 4], 0.5, min_quality=0.25)  # all four frames: 3 of 4 for row 5
    assert ri[0].tolist() == [0, 5, 3, 4, 1, 4, 4, 0] and float(rd[0, 1]) == 0.75
    assert _launch(handle, idx, score, [0, 4], 0.95)[0][0, 0] == 3


def test_track_consensus_argument_errors(handle):
    idx = torch.zeros((8, 2), dtype=torch.int32, device="cuda")
    score = torch.zeros((8, 2), dtype=torch.float32, device="cuda")
    for off in ([1, 8], [0, 0, 8], [0, 9], [0, 3], [0, 5, 4, 8]):
        with pytest.raises(ValueError):
            handle.track_consensus(idx, score, off)
    with pytest.raises(ValueError):
        handle.track_consensus(idx, score, [0, 8], min_frames=0)
    with pytest.raises(ValueError):
        handle.track_consensus(idx.cpu(), score.cpu(), [0, 8])
    with pytest.raises(ValueError):
        handle.track_consensus(idx.float(), score, [0, 8])
    with pytest.raises(ValueError):
        handle.track_consensus(idx[:, :0], score[:, :0], [0, 8])
    big = torch.zeros((1025, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="1025"):
        handle.track_consensus(big, big.float(), [0, 1025])
    ri, rd = handle.track_consensus(idx[:0], score[:0], [0])  # no tracks: a no-op
    assert tuple(ri.shape) == (0, 8) and tuple(rd.shape) == (0, 2)


def test_track_consensus_torch_op(handle, golden_dir):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    g = groups(np.load(os.path.join(golden_dir, "track_consensus.npz")))[1]
    idx, score = torch.from_numpy(g["idx"]).cuda(), torch.from_numpy(g["score"]).cuda()
    off = g["offsets"].tolist()
    ri, rd = torch.ops.frhip.track_consensus(idx, score, off, 0.55, 3, g["similarity_threshold"])
    wi, wd = handle.track_consensus(idx, score, off, 0.55, 3, g["similarity_threshold"])
    assert torch.equal(ri, wi) and torch.equal(rd, wd)
    with FakeTensorMode():
        fi, fd = torch.ops.frhip.track_consensus(torch.empty(9, 3, dtype=torch.int32, device="cuda"),
                                                 torch.empty(9, 3, dtype=torch.float32, device="cuda"),
                                                 [0, 4, 9], 0.55, 3, 0.5)
        assert fi.shape == (2, 8) and fi.dtype == torch.int32 and fi.device.type == "cuda"
        assert fd.shape == (2, 2) and fd.dtype == torch.float64


# ---------------------------------------------------------------- FaceMatcher
@pytest.fixture(scope="module")
def matcher(tmp_path_factory):
    from facerecognitionpipeline_amd import weights as W
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    from facerecognitionpipeline_amd.face_matcher import FaceMatcher
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=64)
    base = W.synthetic_crops(8)
    gm = GalleryManager(gallery_path=str(tmp_path_factory.mktemp("g") / "students.npz"), device=emb.device,
                        verbose=False)
    for i, e in enumerate(emb.extract_embeddings_batch(list(base))):
        gm.add_student(f"S{i:03d}", f"Student {i}", e)
    fm = FaceMatcher(similarity_threshold=0.5, aggregation_method="consensus", architecture="ir_50", embedder=emb,
                     gallery=gm, verbose=False)
    return fm, base


def _tracks(base):
    """6 tracks, 33 frames: one identity (7, 9 and exactly 3 frames), two identities 2 + 2, unrelated
    crops, and an empty track."""
    from facerecognitionpipeline_amd import weights as W

    def probes(i, n, seed):
        return list(W.probe_crops(base[i:i + 1], n, sigma=SIGMA, seed=seed))

    return [probes(0, 7, 11), probes(3, 9, 12), probes(1, 2, 13) + probes(2, 2, 14),
            list(W.synthetic_crops(8, seed=0xBEEF)), [], probes(6, 3, 15)]


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


def test_match_tracks_end_to_end(matcher):
    fm, base = matcher
    tracks = _tracks(base)
    got = fm.match_tracks(tracks, top_k=3)
    flat = fm.match_faces([f for t in tracks for f in t], top_k=3)  # the same launch composition
    assert len(got) == 6 and got[4] is None
    at = 0
    for t, frames in enumerate(tracks):
        if not frames:
            continue
        want_fm = [{"frame": f"{i:06d}", "student_id": m[0][0], "name": m[0][1], "score": m[0][2],
                    "top_k_matches": [{"student_id": s, "name": n, "score": sc} for s, n, sc in m]}
                   for i, m in enumerate(flat[at:at + len(frames)])]
        at += len(frames)
        assert all(len(m["top_k_matches"]) == 3 for m in want_fm)
        _check_decision(fm, got[t], want_fm)
        c = got[t]["consensus"]
        assert c["total_frames_evaluated"] == len(frames) and c["quality_frames"] == len(frames)
        assert (c["status"] == "recognized") == got[t]["recognized"]
    assert [g["recognized"] for g in got if g] == [True, True, False, False, True]
    assert [got[0]["student_id"], got[1]["student_id"], got[5]["student_id"]] == ["S000", "S003", "S006"]
    assert got[0]["name"] == "Student 0" and got[2]["best_candidate"]["student_id"] == "S001"  # first seen of 2 + 2
    assert got[2]["consensus"]["status"] == got[3]["consensus"]["status"] == "no_consensus"
    json.dumps(got)  # plain Python values throughout
    # the threshold is the matcher's: above every score, the same tracks are below_threshold
    fm.similarity_threshold = 1.5
    try:
        high = fm.match_tracks(tracks[:1])
    finally:
        fm.similarity_threshold = 0.5
    assert not high[0]["recognized"] and high[0]["consensus"]["status"] == "below_threshold"
    assert high[0]["best_candidate"]["student_id"] == "S000"


def test_match_tracks_long_track_takes_the_host_vote(matcher):
    """A track of more than 1024 frames (the kernel's limit) is decided by the host statement of the
    vote; the tracks beside it, before and after, still go through the kernel."""
    fm, base = matcher
    tracks = _tracks(base)
    long_track = [tracks[0][i % 7] for i in range(700)] + [tracks[1][i % 9] for i in range(325)]  # 1025 frames
    got = fm.match_tracks([tracks[2], long_track, tracks[5]], top_k=1)
    assert [g["recognized"] for g in got] == [False, True, True]
    assert got[1]["student_id"] == "S000" and got[1]["num_frames"] == 1025
    assert got[1]["consensus"]["winner_frames"] == 700 and got[1]["consensus"]["second_frames"] == 325
    for g in got:
        assert [m["frame"] for m in g["frame_matches"]] == [f"{i:06d}" for i in range(len(g["frame_matches"]))]
        _check_decision(fm, g, g["frame_matches"])
    assert got[2]["student_id"] == "S006" and got[0]["best_candidate"]["student_id"] == "S001"


def test_match_tracks_none_cases(matcher, tmp_path):
    from facerecognitionpipeline_amd.face_matcher import FaceMatcher
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    fm, base = matcher
    assert fm.match_tracks([]) == [] and fm.match_tracks([[], []]) == [None, None]
    empty = GalleryManager(gallery_path=str(tmp_path / "e" / "students.npz"), device=fm.embedder.device, verbose=False)
    fm2 = FaceMatcher(architecture="ir_50", embedder=fm.embedder, gallery=empty, verbose=False)
    try:
        assert fm2.match_tracks([[base[0]], []]) == [None, None]  # an empty gallery matches nothing
    finally:
        fm.gallery.attach_handle(fm.embedder.model)  # fm2 took the shared handle for its gallery


def test_process_capture_directory(matcher, tmp_path):
    from PIL import Image
    from facerecognitionpipeline_amd.face_recognition import load_image_rgb
    fm, base = matcher
    tracks = _tracks(base)
    cap = tmp_path / "camera_captures"
    for t, frames in enumerate(tracks):
        d = cap / f"track_{t:04d}"
        d.mkdir(parents=True)
        (d / "metadata.json").write_text(json.dumps({"track_id": t, "num_frames": len(frames)}))
        for i, f in enumerate(frames):
            Image.fromarray(f, "RGB").save(d / f"face_{i:03d}.jpg", quality=95)
    (cap / "track_0000" / "face_zzz.jpg").write_bytes(b"not a jpeg")     # unreadable: skipped
    (cap / "track_0000" / "notes.png").write_bytes(b"ignored")           # not a .jpg
    (cap / "track_0007").mkdir()                                         # no metadata.json: no result
    Image.fromarray(base[0], "RGB").save(cap / "track_0007" / "face_000.jpg")
    (cap / "other").mkdir()                                              # not a track_* folder
    (cap / "track_file").write_text("a file, not a folder")
    summary = fm.process_capture_directory(str(cap), save_results=True)
    # what match_tracks says about the decoded frames
    names = [sorted(p.name for p in (cap / f"track_{t:04d}").glob("face_[0-9]*.jpg")) for t in range(6)]
    decoded = [[load_image_rgb(str(cap / f"track_{t:04d}" / n)) for n in names[t]] for t in range(6)]
    want = fm.match_tracks(decoded, top_k=3, frame_names=names)
    results = []
    for t in range(6):
        path = cap / f"track_{t:04d}" / "recognition_result.json"
        if want[t] is None:
            assert not path.exists()
            continue
        res = json.loads(path.read_text())
        results.append(res)
        keys = (["track_id", "recognized", "student_id", "name", "confidence", "method", "num_frames"]
                if res["recognized"] else ["track_id", "recognized", "reason", "best_candidate"])
        assert list(res) == keys + ["frame_matches", "metadata", "timestamp"]  # the reference's dict
        assert res["track_id"] == f"track_{t:04d}" and res["metadata"] == {"track_id": t, "num_frames": len(names[t])}
        for k in keys[1:]:
            assert res[k] == want[t][k], (t, k)
        assert res["frame_matches"] == want[t]["frame_matches"]
        assert [m["frame"] for m in res["frame_matches"]] == names[t]
        # match_track alone: the same dict from a launch of this track's frames only (a forward is
        # batch-invariant to ~1e-6, not bit for bit, so it is compared with match_tracks of that launch)
        single = fm.match_track(str(cap / f"track_{t:04d}"))
        alone = fm.match_tracks([decoded[t]], top_k=3, frame_names=[names[t]])[0]
        assert list(single) == list(res) and isinstance(single.pop("timestamp"), str)
        assert (single["track_id"], single["metadata"]) == (res["track_id"], res["metadata"])
        for k in keys[1:] + ["frame_matches"]:
            assert single[k] == alone[k], (t, k)
    assert not (cap / "track_0007" / "recognition_result.json").exists()
    assert fm.match_track(str(cap / "track_0007")) is None and fm.match_track(str(cap / "track_0004")) is None
    on_disk = json.loads((cap / "adaface_ir_50_results" / "recognition_summary.json").read_text())
    n_rec = sum(r["recognized"] for r in results)
    ref = fm._generate_summary(results, n_rec, len(results) - n_rec)
    for s in (summary, on_disk):
        assert {k: v for k, v in s.items() if k != "timestamp"} == {k: v for k, v in ref.items() if k != "timestamp"}
    assert summary["total_tracks"] == 5 and summary["recognized"] == n_rec >= 1 and summary["unrecognized"] >= 1
    assert summary["settings"] == {"similarity_threshold": 0.5, "aggregation_method": "consensus"}
    # the reference's other two outcomes
    assert fm.process_capture_directory(str(cap / "other"), save_results=False) == {"error": "no_tracks"}
    with pytest.raises(ValueError, match="Capture directory not found"):
        fm.process_capture_directory(str(cap / "missing"))
