"""GPU: ``fr_server_tracks`` against the reference's outputs (tests/golden/server_tracks.npz) and the
host statement of its contract (``server_tracks_host``): the three arrays and the track records exact;
the launch shapes at which the kernel takes another path, its limits, its torch op;
``FaceRecognitionServer.process_requests`` / ``process_frames`` against this module's per-request
``process_faces`` / ``process_full_frame`` loops on a replayed detector."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import _live_cases as LC
from tests import _server_cases as SC
from tests.test_gpu_capture_tracks import QUALITY, ReplayDetector, _face
from tests.test_gpu_live_tracks import H, THRESHOLD, W, _same, _stamps, models  # noqa: F401  (models: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=1)  # never finalised


def _launch(handle, metrics, clock, order, offsets, **kw):
    out = handle.server_tracks(torch.from_numpy(np.ascontiguousarray(metrics, np.float64)).cuda(),
                               torch.from_numpy(np.ascontiguousarray(clock, np.float64)).cuda(),
                               torch.from_numpy(np.ascontiguousarray(order, np.int32)).cuda(), offsets, **kw)
    assert all(x.dtype == torch.int32 and x.is_cuda for x in out)
    return tuple(x.cpu().numpy() for x in out)


def _assert_equal(got, want, label):
    for name, g, w in zip(("attempt", "best", "state", "track_info"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (label, name, np.flatnonzero((g != w).reshape(len(g), -1)
                                                                                         .any(axis=1))[:8])


def test_server_tracks_matches_the_reference_and_the_host_statement(handle, golden_dir):
    from facerecognitionpipeline_amd.face_recognition_server import resolve_server_attempts, server_tracks_host
    reached = set()
    gallery = LC.HostGallery()
    for k, s in enumerate(SC.sessions(np.load(os.path.join(golden_dir, "server_tracks.npz")))):
        per_det, order, offsets, _keys = SC.grouped(s)
        got = _launch(handle, s["metrics"], per_det, order, offsets, **s["kernel"])
        print(k, got[3][:, :3].sum(axis=0).tolist())
        trace = set()
        _assert_equal(got, server_tracks_host(s["metrics"], per_det, order, offsets, trace=trace, **s["kernel"]), k)
        # the reference's outputs: its attempts out of the kernel's candidates
        log, _events = resolve_server_attempts(s["ids"].tolist(), got[0], got[1], LC.recognise_with(s, gallery),
                                               s["similarity_threshold"], s["kernel"]["max_attempts"], trace=trace)
        assert [[e["det"], e["track"], e["attempt"], e["best"]] for e in log] == s["log"].tolist(), k
        assert len(log) == s["statistics"]["total_recognition_attempts"], k
        reached |= trace
    # the other four are named by the server's request flows
    assert reached >= SC.REQUIRED - {"track_twice_in_request", "empty_request", "second_track_higher",
                                     "second_track_lower"}


BLOCKED = dict(det=(0.6, 0.6, 0.7, 0.9), blur=(260.0, 30.0, 30.0, 30.0))  # long gated runs: the window fills up
SHAPES = {
    "1 track": (dict(lengths=[9]), {}),
    "63 tracks": (dict(lengths=list(range(1, 13)) * 5 + [3, 2, 1]), {}),
    "64 tracks": (dict(lengths=list(range(1, 17)) * 4), {}),
    "65 tracks": (dict(lengths=[1] + list(range(1, 17)) * 4), {}),
    "1000 tracks": (dict(lengths=[1 + i % 7 for i in range(1000)]), dict(max_attempts=2, retry_cooldown=2.0)),
    "1 and 300": (dict(lengths=[1, 300, 5]), dict(retry_cooldown=4.0)),
    "buffer 1": (dict(lengths=[300, 64, 65, 1]), dict(buffer_size=1)),
    "buffer 2": (dict(lengths=[300, 64, 65, 1]), dict(buffer_size=2, retry_cooldown=1.0)),
    "buffer 63": (dict(lengths=[300, 63, 64, 65, 127, 129], **BLOCKED), dict(buffer_size=63, max_attempts=16)),
    "buffer 64": (dict(lengths=[300, 63, 64, 65, 127, 129], **BLOCKED), dict(buffer_size=64, max_attempts=16)),
    "buffer 64 attempts": (dict(lengths=[300, 128, 70]), dict(buffer_size=64, max_attempts=16, retry_cooldown=30.0)),
    "max_attempts 1": (dict(lengths=[40, 20, 1, 7]), dict(max_attempts=1, retry_cooldown=1.0)),
    "max_attempts 16": (dict(lengths=[200, 20, 1, 7]), dict(max_attempts=16, retry_cooldown=5.0)),
    "retry_cooldown 0": (dict(lengths=[80, 20, 1, 7], clock_steps=(0.0, 0.0, 0.5)), dict(retry_cooldown=0.0)),
    "fresh ids": (dict(lengths=[1] * 200), {}),
    "one track": (dict(lengths=[500]), dict(retry_cooldown=3.0)),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_seeded_logs_against_the_host_statement(handle, name):
    from facerecognitionpipeline_amd.face_recognition_server import SERVER_ATTEMPT, SERVER_RESET, server_tracks_host
    log_kw, kernel_kw = SHAPES[name]
    params = dict(max_attempts=3, buffer_size=10, retry_cooldown=10.0, det_gate=0.6)
    params.update(kernel_kw)
    metrics, clock, order, offsets = SC.random_tracks(0x5EED + len(name), **log_kw)
    got = _launch(handle, metrics, clock, order, offsets, **params)
    want = server_tracks_host(metrics, clock, order, offsets, **params)
    print(name, "detections", len(clock), "attempts / cooldowns / resets", got[3][:, :3].sum(axis=0).tolist())
    _assert_equal(got, want, name)
    assert (got[2] == SERVER_ATTEMPT).any()
    if name not in ("1 track", "fresh ids"):
        assert (got[2] == SERVER_RESET).any() or params["max_attempts"] == 16
    again = _launch(handle, metrics, clock, order, offsets, **params)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))  # deterministic


@pytest.mark.parametrize("buffer_size", [1, 2, 63, 64])
def test_the_window_ends_exactly_at_buffer_size(handle, buffer_size):
    """A face at the gate with the largest key, then 139 faces over the gate with a smaller one: the
    first blocks the others for as long as it is in the window, across the chunk boundary at 64."""
    from facerecognitionpipeline_amd.face_recognition_server import server_tracks_host
    metrics = np.array([[0.6, 260.0]] + [[0.9, 30.0]] * 139)
    clock = np.arange(140.0)
    params = dict(max_attempts=16, buffer_size=buffer_size, retry_cooldown=1000.0, det_gate=0.6)
    got = _launch(handle, metrics, clock, np.arange(140), [0, 140], **params)
    _assert_equal(got, server_tracks_host(metrics, clock, np.arange(140), [0, 140], **params), buffer_size)
    tried = np.flatnonzero(got[0] >= 0)
    assert tried.tolist() == list(range(buffer_size, buffer_size + 16)) and got[3].tolist() == [[16, 1, 0, 0]]
    # equal keys: the oldest face of the window, which moves on by one per step
    assert got[1][tried].tolist() == [max(1, d - buffer_size + 1) for d in tried]


def test_a_track_with_a_non_finite_value_is_reported_and_the_others_stay_intact(handle):
    from facerecognitionpipeline_amd import face_recognition_server as S
    metrics, clock, order, offsets = SC.random_tracks(0xBAD, [70, 9, 130, 4])
    params = dict(max_attempts=3, buffer_size=10, retry_cooldown=2.0, det_gate=0.6)
    clean = S.server_tracks_host(metrics, clock, order, offsets, **params)
    for what, column in (("blur", 1), ("det", 0), ("clock", None)):
        m, c = metrics.copy(), clock.copy()
        spot = int(order[offsets[2] + 67])  # track 2, in its second chunk of 64
        if column is None:
            c[spot] = np.inf
        else:
            m[spot, column] = np.nan
        with pytest.raises(NotImplementedError, match="track 2: a non-finite metric or clock"):
            _launch(handle, m, c, order, offsets, **params)
        attempt, best, state, info = _launch(handle, m, c, order, offsets, raise_on_track_error=False, **params)
        _assert_equal((attempt, best, state, info), S.server_tracks_host(m, c, order, offsets, **params), what)
        assert info[2].tolist() == [0, 0, 0, S.SERVER_ERR_VALUE]
        mine = order[offsets[2]:offsets[3]]
        assert (attempt[mine] == -1).all() and (best[mine] == -1).all() and (state[mine] == S.SERVER_GATED).all()
        others = np.setdiff1d(np.arange(len(clock)), mine)
        assert all(np.array_equal(g[others], w[others]) for g, w in zip((attempt, best, state), clean))
        assert np.array_equal(info[[0, 1, 3]], clean[3][[0, 1, 3]]) and info[[0, 1, 3], 0].sum() > 0
    # an order entry past the detections: reported, nothing written out of range
    bad = order.copy()
    bad[offsets[1] + 2] = len(clock)
    with pytest.raises(NotImplementedError, match="track 1: an order entry outside"):
        _launch(handle, metrics, clock, bad, offsets, **params)
    got = _launch(handle, metrics, clock, bad, offsets, raise_on_track_error=False, **params)
    _assert_equal(got, S.server_tracks_host(metrics, clock, bad, offsets, **params), "order")
    assert got[3][1].tolist() == [0, 0, 0, S.SERVER_ERR_ORDER]


def test_server_tracks_argument_errors(handle):
    from facerecognitionpipeline_amd import _lib
    metrics = torch.zeros((8, 2), dtype=torch.float64, device="cuda")
    clock = torch.zeros((8,), dtype=torch.float64, device="cuda")
    order = torch.arange(8, dtype=torch.int32, device="cuda")
    for off in ([1, 8], [0, 9], [0, 5, 4, 8], [0, 7], []):
        with pytest.raises(ValueError):
            handle.server_tracks(metrics, clock, order, off)
    for kw in ({"max_attempts": 0}, {"max_attempts": 17}, {"buffer_size": 0}, {"buffer_size": 65},
               {"retry_cooldown": -1.0}, {"retry_cooldown": float("nan")}, {"retry_cooldown": float("inf")},
               {"det_gate": float("nan")}, {"det_gate": float("inf")}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            handle.server_tracks(metrics, clock, order, [0, 8], **kw)
    with pytest.raises(ValueError):
        handle.server_tracks(metrics.cpu(), clock.cpu(), order.cpu(), [0, 8])
    for m, c, o in ((metrics.float(), clock, order), (metrics, clock.float(), order), (metrics, clock, order.long()),
                    (metrics, clock[:7], order), (metrics[:, :1], clock, order)):
        with pytest.raises(ValueError):
            handle.server_tracks(m, c, o, [0, 8])
    # the C entry point: every check with the handle and without it
    lib = _lib.load()
    outs = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in range(3)]
    info = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    off = (ctypes.c_int32 * 3)(0, 3, 8)
    down = (ctypes.c_int32 * 3)(0, 5, 3)

    def call(h, metrics=metrics, clock=clock, order=order, off=off, n_tracks=2, n_dets=8, max_attempts=3,
             buffer_size=10, retry_cooldown=10.0, det_gate=0.6, skip=None, info=info):
        o = [None if i == skip else _lib.ptr(x) for i, x in enumerate(outs)]
        rc = lib.fr_server_tracks(h, _lib.ptr(metrics), _lib.ptr(clock), _lib.ptr(order), off, n_tracks, n_dets,
                                  max_attempts, buffer_size, retry_cooldown, det_gate, o[0], o[1], o[2],
                                  _lib.ptr(info), None)
        return rc, lib.fr_last_error(h)

    for h in (None, handle.h):
        for kw, text in (({"metrics": None}, b"NULL buffer"), ({"clock": None}, b"NULL buffer"),
                         ({"order": None}, b"NULL buffer"), ({"off": None}, b"NULL buffer"),
                         ({"skip": 0}, b"NULL buffer"), ({"skip": 1}, b"NULL buffer"), ({"skip": 2}, b"NULL buffer"),
                         ({"info": None}, b"NULL buffer"), ({"n_tracks": -1}, b"n_tracks"), ({"n_dets": -1}, b"n_dets"),
                         ({"off": down}, b"track_offsets decrease at track 1"), ({"max_attempts": 17}, b"max_attempts"),
                         ({"buffer_size": 65}, b"buffer_size"), ({"retry_cooldown": -1.0}, b"retry_cooldown"),
                         ({"det_gate": float("nan")}, b"det_gate")):
            rc, msg = call(h, **kw)
            assert rc == _lib.FR_ERR_INVALID_ARGUMENT and text in msg, (h, kw, msg)
    assert call(None)[1] == b"NULL handle" and call(handle.h)[0] == _lib.FR_OK
    # the one call that ran found every face gated (det_score 0)
    assert [x.cpu().unique().tolist() for x in outs] == [[-1], [-1], [0]] and not info.any().item()
    out = handle.server_tracks(metrics[:0], clock[:0], order[:0], [0])  # no tracks: a no-op
    assert [tuple(x.shape) for x in out] == [(0,), (0,), (0,), (0, 4)]
    out = handle.server_tracks(metrics, clock, order[:3], [0, 0, 3, 3])  # tracks without appearances
    assert out[3].cpu().tolist() == [[0, 0, 0, 0]] * 3 and out[0].cpu().tolist() == [-1] * 8


def test_server_tracks_torch_op(handle, golden_dir):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    s = SC.sessions(np.load(os.path.join(golden_dir, "server_tracks.npz")))[0]
    per_det, order, offsets, _keys = SC.grouped(s)
    k = s["kernel"]
    args = (torch.from_numpy(s["metrics"]).cuda(), torch.from_numpy(per_det).cuda(), torch.from_numpy(order).cuda())
    got = torch.ops.frhip.server_tracks(*args, offsets.tolist(), k["max_attempts"], k["buffer_size"],
                                        k["retry_cooldown"], 0.6)
    want = handle.server_tracks(*args, offsets, **k)
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert int((got[0] >= 0).sum()) >= len(s["log"]) > 0
    with FakeTensorMode():
        out = torch.ops.frhip.server_tracks(torch.empty(9, 2, dtype=torch.float64, device="cuda"),
                                            torch.empty(9, dtype=torch.float64, device="cuda"),
                                            torch.empty(9, dtype=torch.int32, device="cuda"), [0, 4, 4, 9], 3, 10,
                                            10.0, 0.6)
        assert [tuple(x.shape) for x in out] == [(9,), (9,), (9,), (3, 4)]
        assert all(x.dtype == torch.int32 and x.device.type == "cuda" for x in out)


# ---------------------------------------------------------------- FaceRecognitionServer
N_FRAMES = 14
STEP = 1.5  # seconds between requests: three failures, a cooldown of 10 s, a reset and a second cycle in 14 requests


def _scene(seed):
    """A static noise scene (every crop is sharp) with a smooth band, in RGB, and the people of its
    frames as (client id, face): 0, 2 and 3 stand still at the places the gallery's templates were
    made from (A: cosine 1, C: 0.981, under THRESHOLD, D: 0.995), 1 walks, 3 is away on frame 6, 4
    arrives late, 5 shows up on the smooth band."""
    r = np.random.Generator(np.random.PCG64(seed))
    scene = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    scene[170:, :, :] = 128
    rgb = np.ascontiguousarray(scene[..., ::-1])
    people = []
    for k in range(N_FRAMES):
        faces = [(0, _face(60, 60, 0.9)), (1, _face(150 + 5 * k, 70 + 2 * k, 0.7 + 0.02 * (k % 5), roll=0.1)),
                 (2, _face(330, 60, 0.8))]
        if k not in (0, 6):
            faces.append((3, _face(250, 120, 0.85)))
        if k >= 9:
            faces.append((4, _face(40, 130, 0.75)))
        if k % 3 == 0:
            faces.append((5, _face(120 + 10 * k, 200, 0.95)))
        people.append([faces[j] for j in r.permutation(len(faces))])
    return [rgb] * N_FRAMES, people


def _server(models, per_frame, out_dir, clock, **kw):
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    from facerecognitionpipeline_amd.face_recognition_server import FaceRecognitionServer
    emb, gm = models
    proc = FaceProcessor(output_size=112, detector=ReplayDetector(per_frame), quality_filter_config=QUALITY,
                         device=torch.device("cuda", 0))
    settings = dict(max_recognition_attempts=3, frame_buffer_size=3, retry_cooldown=10.0)
    settings.update(kw)
    return FaceRecognitionServer(similarity_threshold=THRESHOLD, output_dir=str(out_dir), session_name="s",
                                 processor=proc, embedder=emb, gallery=gm, clock=lambda: clock[0], verbose=False,
                                 **settings)


def _watch_scores(server, scores):
    inner = server._result_of

    def result_of(matches, *a, **kw):
        scores.append(matches[0][2])
        return inner(matches, *a, **kw)

    server._result_of = result_of


def _assert_servers_equal(a, b):
    with open(os.path.join(a.session_dir, "attendance.json")) as f, open(os.path.join(b.session_dir,
                                                                                      "attendance.json")) as g:
        att_a, att_b = json.load(f), json.load(g)
    _same(att_a, att_b, "attendance")
    for entry in att_a["recognized"] + att_a["unrecognized"] + att_b["recognized"] + att_b["unrecognized"]:
        assert os.path.exists(entry["saved_face_path"])
    ta, tb = a.tracker, b.tracker
    assert ta.recognition_attempts == tb.recognition_attempts and ta.track_cooldowns == tb.track_cooldowns
    assert list(ta.recognized_tracks) == list(tb.recognized_tracks)
    _same({k: dict(v) for k, v in ta.recognized_tracks.items()}, {k: dict(v) for k, v in tb.recognized_tracks.items()})
    assert ta.track_first_seen == tb.track_first_seen and ta.track_last_seen == tb.track_last_seen
    assert list(ta.track_last_attempt) == list(tb.track_last_attempt)
    assert {k: len(v) for k, v in ta.track_frame_buffers.items()} == {k: len(v) for k, v in
                                                                      tb.track_frame_buffers.items()}
    assert (a.frame_count, a.total_faces_detected, a.total_recognition_attempts, a.next_track_id) == (
        b.frame_count, b.total_faces_detected, b.total_recognition_attempts, b.next_track_id)
    sa, sb = a.finalize_session(), b.finalize_session()
    assert sa["statistics"] == sb["statistics"] and sa["settings"] == sb["settings"]
    return att_a, sa["statistics"]


def test_process_frames_equals_the_process_full_frame_loop(models, tmp_path):
    frames, people = _scene(0x11FE)
    per_frame = [[f for _id, f in faces] for faces in people]
    clocks = [STEP * i for i in range(N_FRAMES)]
    stamps = _stamps(N_FRAMES)
    now, scores = [0.0], []
    loop = _server(models, per_frame, tmp_path / "loop", now)
    _watch_scores(loop, scores)
    loop_results = []
    for i, frame in enumerate(frames):
        now[0] = clocks[i]
        loop_results.append(loop.process_full_frame(frame, i + 1, stamps[i]))
    print("top-1 scores", sorted(round(s, 4) for s in scores))
    # no decision of the per-request flow is within reach of the batched flow's last bits
    assert all(abs(s - THRESHOLD) > 1e-4 for s in scores)
    batched = _server(models, per_frame, tmp_path / "batched", [0.0])
    calls = []
    inner = batched._search_faces
    batched._search_faces = lambda faces: (calls.append(len(faces)), inner(faces))[1]
    results = batched.process_frames(frames, list(range(1, N_FRAMES + 1)), stamps, clocks)
    _same(loop_results, results, "results")
    attendance, stats = _assert_servers_equal(loop, batched)
    print(stats, calls)
    assert calls == [stats["total_recognition_attempts"]] == [len(scores)]  # one embed + match batch for the log
    n_faces = sum(len(f) for f in per_frame)
    assert batched.next_track_id == n_faces and stats["total_recognition_attempts"] == n_faces  # all over the gate
    assert [s["student_id"] for s in attendance["recognized"]] == ["S000", "S001"]
    assert abs(attendance["recognized"][0]["confidence"] - 1.0) < 1e-5 and attendance["unrecognized"] == []
    assert len(batched.tracker.recognized_tracks) == N_FRAMES + (N_FRAMES - 2)  # A on every frame, D on twelve
    for entry in attendance["recognized"]:
        assert os.path.exists(entry["saved_face_path"].replace("_aligned.png", "_original.png"))


def test_process_requests_equals_the_process_faces_loop(models, tmp_path):
    from facerecognitionpipeline_amd.face_recognition_server import encode_png
    frames, people = _scene(0x11FE)
    per_frame = [[f for _id, f in faces] for faces in people]
    # the client's side: detect and align every frame, name the faces by their people
    client = _server(models, per_frame, tmp_path / "client", [0.0]).face_processor
    requests = []
    for k, (frame, faces) in enumerate(zip(frames, people)):
        found = client.process_numpy(frame, return_all=True)
        ids = {tuple(f["bbox"].tolist()): pid for pid, f in faces}
        body = [{"track_id": ids[tuple(np.asarray(f["bbox"]).astype(np.int32).tolist())],
                 "bbox": [float(x) for x in f["bbox"]], "det_score": float(f["det_score"]),
                 "quality_metrics": {q: float(v) if isinstance(v, (np.integer, np.floating)) else v
                                     for q, v in f["quality_metrics"].items()},
                 "aligned_face_base64": encode_png(f["aligned_face"])} for f in found]
        if k == 4:
            body.append(dict(body[0]))  # a track twice in one request
        requests.append({"faces": body, "frame_count": k + 1})
    requests.insert(5, {"faces": [], "frame_count": 99})  # an empty request
    clocks = [STEP * i for i in range(len(requests))]
    stamps = _stamps(len(requests))
    now, scores = [0.0], []
    loop = _server(models, per_frame, tmp_path / "loop", now)
    _watch_scores(loop, scores)
    loop_results = []
    for i, request in enumerate(requests):
        now[0] = clocks[i]
        loop_results.append(loop.process_faces(request["faces"], request["frame_count"], timestamp=stamps[i]))
    print("top-1 scores", sorted(round(s, 4) for s in scores))
    assert all(abs(s - THRESHOLD) > 1e-4 for s in scores)
    batched = _server(models, per_frame, tmp_path / "batched", [0.0])
    batched.trace = set()
    calls = []
    inner = batched._search_faces
    batched._search_faces = lambda faces: (calls.append(len(faces)), inner(faces))[1]
    results = batched.process_requests(requests, clocks, timestamps=stamps)
    _same(loop_results, results, "results")
    attendance, stats = _assert_servers_equal(loop, batched)
    print(stats, calls, batched.last_track_info.tolist())
    assert sum(calls) == stats["total_recognition_attempts"] == len(scores) and len(calls) <= 6 < len(scores)
    assert batched.trace >= {"track_twice_in_request", "empty_request"}
    # what the log was built to show: A and D recognised at once, C given up on in two cooldown cycles
    assert [s["student_id"] for s in attendance["recognized"]] == ["S000", "S001"]
    by_track = {}
    for u in attendance["unrecognized"]:
        by_track.setdefault(u["track_id"], []).append(u)
    assert len(by_track["track_0002"]) == 2 and by_track["track_0002"][0]["best_match"]["student_id"] == "S002"
    assert all(u["attempts"] == 3 and len(u["top_matches"]) == 3 for u in attendance["unrecognized"])
    assert batched.last_track_info[:, 2].sum() >= 1 and batched.tracker.track_cooldowns  # resets; one still cooling
    assert stats["total_recognition_attempts"] < int(batched.last_track_info[:, 0].sum())  # dropped after a success
    with pytest.raises(RuntimeError, match="whole session"):
        batched.process_requests(requests, clocks)
