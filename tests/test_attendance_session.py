"""CPU-only: what attendance_session.py holds for the live loop and the server: the class tree, the
resolver core behind resolve_attempts / resolve_server_attempts, and what a session prints (the
transcripts below were recorded before the two classes got their shared base)."""
import os
import re

import numpy as np

from tests import _live_cases as LC
from tests import _server_cases as SC

RULE = "=" * 70

LIVE_TRANSCRIPT = f"""
{RULE}
INITIALIZING LIVE FACE RECOGNITION SYSTEM
{RULE}
Loaded 5 enrolled students

{RULE}
System ready!
Session: live_1
Output: <DIR>/live_1
Recognition interval: every 2 frames
Similarity threshold: 0.5
{RULE}

[Frame 2] Below threshold: Student 0 (track_0000, confidence: 0.300, threshold: 0.5)
[Frame 2] Below threshold: Student 1 (track_0001, confidence: 0.310, threshold: 0.5)
[Frame 4] Recognized: Student 0 (track_0000, confidence: 0.700)
[Frame 4] Below threshold: Student 1 (track_0001, confidence: 0.310, threshold: 0.5)
[Frame 6] Below threshold: Student 1 (track_0001, confidence: 0.330, threshold: 0.5)
[Frame 6] Recognized: Student 0 (track_0002, confidence: 0.900)
[Frame 8] Recognized: Student 0 (track_0003, confidence: 0.600)
[Frame 12] Below threshold: Student 2 (track_0004, confidence: 0.400, threshold: 0.5)
[Frame 14] Below threshold: Student 2 (track_0004, confidence: 0.400, threshold: 0.5)

{RULE}
FINALIZING SESSION
{RULE}

Session: live_1
Duration: <S> seconds
Frames processed: 14
Average FPS: <F>

Recognized students: 1
Student 0 (S000) - confidence: 0.900

Unrecognized tracks: 1
track_0001 - best match: Student 1 (0.330)

Output directory: <DIR>/live_1
{RULE}

"""

SERVER_TRANSCRIPT = f"""
{RULE}
INITIALIZING FACE RECOGNITION SERVER
{RULE}
Loaded 5 enrolled students

{RULE}
Session created: server_1
Output: <DIR>/server_1
{RULE}

[Frame 1] Below threshold: Student 0 (track_0001, confidence: 0.300, threshold: 0.5)
[Frame 4] Below threshold: Student 2 (track_0001, confidence: 0.450, threshold: 0.5)
[Frame 5] Recognized: Student 1 (track_0002, confidence: 0.900)

{RULE}
FINALIZING SESSION
{RULE}

Session: server_1
Duration: <S> seconds
Frames processed: 6

Recognized students: 1
  Student 1 (S001) - confidence: 0.900

Unrecognized tracks: 2
  track_0001 - best match: Student 0 (0.300)
  track_0001 - best match: Student 2 (0.450)

Output directory: <DIR>/server_1
{RULE}

"""

NO_SESSION_TRANSCRIPT = f"""
{RULE}
INITIALIZING FACE RECOGNITION SERVER
{RULE}
Loaded 0 enrolled students

WARNING: Gallery is empty! Please enroll students first.

{RULE}
Server ready!
Waiting for client to initialize session...
Recognition interval: every 30 frames
Similarity threshold: 0.5
{RULE}

"""


def _masked(text, out_dir):
    text = text.replace(str(out_dir), "<DIR>")
    text = re.sub(r"Duration: [\d.]+ seconds", "Duration: <S> seconds", text)
    return re.sub(r"Average FPS: [\d.]+", "Average FPS: <F>", text)


def test_the_mirrors_subclass_the_shared_bases():
    from facerecognitionpipeline_amd import attendance_session as A
    from facerecognitionpipeline_amd import face_recognition_live as L
    from facerecognitionpipeline_amd import face_recognition_server as S
    assert issubclass(L.LiveRecognitionTracker, A.TrackRecords) and issubclass(S.LiveRecognitionTracker, A.TrackRecords)
    assert issubclass(L.LiveFaceRecognition, A.AttendanceSession)
    assert issubclass(S.FaceRecognitionServer, A.AttendanceSession)
    assert L.selection_key is A.selection_key
    assert L.LiveFaceRecognition.PROCESSOR_CONFIG is S.FaceRecognitionServer.PROCESSOR_CONFIG is A.PROCESSOR_CONFIG
    # what is each class's own is not in the bases
    for name in ("should_recognize", "is_track_in_cooldown", "set_track_cooldown", "end_cooldown"):
        assert not hasattr(A.TrackRecords, name), name
    for name in ("_settle", "_save_face_image", "_finalize_session", "finalize_session"):
        assert not hasattr(A.AttendanceSession, name), name


def test_resolver_core_with_explicit_ordinals_against_both_wrappers():
    from facerecognitionpipeline_amd.attendance_session import _resolve
    from facerecognitionpipeline_amd.face_recognition_live import resolve_attempts
    from facerecognitionpipeline_amd.face_recognition_server import resolve_server_attempts

    def recogniser(calls):
        def recognise(dets):
            calls.append(list(dets))
            return [[("S", "n", 0.9 if d == 14 else 0.1)] for d in dets]
        return recognise

    def nobody(dets):
        return [[] for _ in dets]

    # the inputs of test_resolve_server_attempts_cycles_and_an_empty_gallery
    keys = ["a", "b", "a", "b", "a", "b", "a"]
    attempt, best = [0, 0, 1, 1, 2, 2, 3], [10, 11, 12, 14, 10, 11, 12]
    for ordinals, wrapper in (([0, 1, 2, 3], resolve_server_attempts), ([0, 1], resolve_attempts)):
        calls, wrapper_calls, trace, wrapper_trace = [], [], set(), set()
        got = _resolve(ordinals, keys, attempt, best, recogniser(calls), 0.5, 2, trace)
        assert got == wrapper(keys, attempt, best, recogniser(wrapper_calls), 0.5, 2, wrapper_trace)
        assert calls == wrapper_calls and trace == wrapper_trace - {"unfinished_track"}
        assert _resolve(ordinals, [0, 0, 0], [0, 1, -1], [0, 0, -1], nobody, 0.5, 2) == wrapper(
            [0, 0, 0], [0, 1, -1], [0, 0, -1], nobody, 0.5, 2)
    # every ordinal present: both cycles of track "a"; the ordinals of one cycle: the first alone
    log, events = _resolve([0, 1, 2, 3], keys, attempt, best, recogniser([]), 0.5, 2)
    assert [(e["det"], e["type"]) for e in events] == [(2, "unrecognized"), (3, "recognized"), (6, "unrecognized")]
    log, events = _resolve([0, 1], keys, attempt, best, recogniser([]), 0.5, 2)
    assert [(e["det"], e["attempt"]) for e in log] == [(0, 0), (1, 0), (2, 1), (3, 1)]
    assert [(e["det"], e["type"]) for e in events] == [(2, "unrecognized"), (3, "recognized")]
    # the ordinals are visited in the order given
    calls = []
    _resolve([1, 0], keys, attempt, best, recogniser(calls), 0.5, 2)
    assert calls == [[12, 14], [10]]


def test_what_a_session_prints(golden_dir, tmp_path, capsys):
    """The banners, the per-attempt lines and the closing summary of either class: live has the
    "System ready!" banner and the FPS line and does not indent the summary's entries; the server has
    the "Session created" banner and indents them by two spaces."""
    from facerecognitionpipeline_amd.face_recognition_live import LiveFaceRecognition
    from facerecognitionpipeline_amd.face_recognition_server import FaceRecognitionServer
    s = LC.sessions(np.load(os.path.join(golden_dir, "live_tracks.npz")))[1]
    k = s["kernel"]
    live = LiveFaceRecognition(similarity_threshold=s["similarity_threshold"], output_dir=str(tmp_path),
                               session_name="live_1", recognition_interval=k["recognition_interval"],
                               max_recognition_attempts=k["max_attempts"], frame_buffer_size=k["buffer_size"],
                               processor=LC.ReplayProcessor(s), embedder=LC.PlanEmbedder(s), gallery=LC.HostGallery())
    live.max_distance = k["max_distance"]
    LC.drive(live, s)
    live._finalize_session()
    assert _masked(capsys.readouterr().out, tmp_path) == LIVE_TRANSCRIPT

    s = SC.sessions(np.load(os.path.join(golden_dir, "server_tracks.npz")))[1]
    k = s["kernel"]
    clock = [0.0]
    srv = FaceRecognitionServer(similarity_threshold=s["similarity_threshold"], output_dir=str(tmp_path),
                                session_name="server_1", max_recognition_attempts=k["max_attempts"],
                                frame_buffer_size=k["buffer_size"], retry_cooldown=k["retry_cooldown"],
                                clock=lambda: clock[0], processor=SC.ReplayProcessor(s), embedder=LC.PlanEmbedder(s),
                                gallery=LC.HostGallery())
    SC.drive(srv, s, lambda seconds: clock.__setitem__(0, seconds))
    srv.finalize_session()
    assert _masked(capsys.readouterr().out, tmp_path) == SERVER_TRANSCRIPT

    class EmptyGallery(LC.HostGallery):
        def get_all_students(self):
            return {}

    FaceRecognitionServer(output_dir=str(tmp_path), processor=object(), embedder=LC.PlanEmbedder({}),
                          gallery=EmptyGallery())
    assert capsys.readouterr().out == NO_SESSION_TRANSCRIPT
