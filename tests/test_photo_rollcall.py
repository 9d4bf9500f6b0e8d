"""CPU: ``photo_rollcall_host`` (the host statement of ``fr_photo_rollcall``) against a brute-force
definition of the exclusive rule, the reference's one-line rule, and the rule's invariants.  Cases:
tests/_rollcall_cases.py."""
import numpy as np
import pytest

from tests import _rollcall_cases as RC

CASES = RC.cases()


@pytest.fixture(scope="module")
def host():
    from facerecognitionpipeline_amd.face_matcher import photo_rollcall_host
    return photo_rollcall_host


@pytest.mark.parametrize("name", sorted(CASES))
def test_exclusive_equals_repeated_argmax(host, name):
    c = CASES[name]
    for thr in RC.THRESHOLDS:
        got = host(c["idx"], c["score"], c["offsets"], thr, RC.EXCLUSIVE)
        assert RC.same(got, RC.exclusive_brute_force(c["idx"], c["score"], c["offsets"], thr)), (name, thr)


@pytest.mark.parametrize("name", sorted(CASES))
def test_independent_is_the_reference_rule(host, name):
    c = CASES[name]
    for thr in RC.THRESHOLDS:
        got = host(c["idx"], c["score"], c["offsets"], thr, RC.INDEPENDENT)
        assert RC.same(got, RC.independent_rule(c["idx"], c["score"], c["offsets"], thr)), (name, thr)


@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants(host, name):
    c = CASES[name]
    idx, score, off = c["idx"], c["score"], c["offsets"]
    for thr in RC.THRESHOLDS:
        face, fscore, image = host(idx, score, off, thr, RC.EXCLUSIVE)
        ind = host(idx, score, off, thr, RC.INDEPENDENT)[0]
        assert face.dtype == np.int32 and fscore.dtype == np.float32 and image.dtype == np.int32
        assert image.shape == (len(off) - 1, 4) and np.array_equal(image[:, 0], np.diff(off))
        assert np.array_equal(image[:, 1:].sum(axis=1), image[:, 0])  # the counts add up to n_faces
        for p, (a, b) in enumerate(zip(off[:-1], off[1:])):
            rec = face[a:b, 0] == RC.RECOGNIZED
            rows = face[a:b, 1][rec]
            assert len(set(rows.tolist())) == len(rows), (name, thr, p)  # no row is granted twice
            assert [int((face[a:b, 0] == s).sum()) for s in (0, 1, 2)] == image[p, 1:].tolist()
        # the reported row and score are the face's own, at the reported column
        at = np.arange(len(face))
        assert np.array_equal(idx[at, face[:, 2]], face[:, 1])
        assert score[at, face[:, 2]].tobytes() == fscore.tobytes()
        assert not face[:, 3].any() and not face[face[:, 0] != RC.RECOGNIZED, 2].any()
        with np.errstate(invalid="ignore"):
            assert (fscore[face[:, 0] == RC.RECOGNIZED].astype(np.float64) >= thr).all()
        # only a face the reference's rule recognises can be displaced, and whoever it does not stays a
        # candidate unless a later column of it is a claim
        assert (ind[face[:, 0] == RC.DISPLACED, 0] == RC.RECOGNIZED).all()


def test_fr_photo_rollcall_argument_errors_without_gpu():
    """The argument checks come before the handle, so they are reported for a NULL handle too."""
    import ctypes
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    n = 8
    idx, out_face = (ctypes.c_int32 * (2 * n))(), (ctypes.c_int32 * (4 * n))()
    score, out_score = (ctypes.c_float * (2 * n))(), (ctypes.c_float * n)()
    out_image = (ctypes.c_int32 * 8)()

    def call(idx=idx, score=score, k=2, offsets=(0, 3, 8), n_images=2, thr=0.5, mode=0, out_face=out_face,
             out_score=out_score, out_image=out_image):
        off = (ctypes.c_int32 * len(offsets))(*offsets) if offsets is not None else None
        rc = lib.fr_photo_rollcall(None, idx, score, k, off, n_images, thr, mode, out_face, out_score, out_image, None)
        return rc, lib.fr_last_error(None)

    for kw, text in (({}, b"NULL handle"), ({"idx": None}, b"NULL buffer"), ({"score": None}, b"NULL buffer"),
                     ({"offsets": None}, b"NULL buffer"), ({"out_face": None}, b"NULL buffer"),
                     ({"out_score": None}, b"NULL buffer"), ({"out_image": None}, b"NULL buffer"),
                     ({"n_images": -1}, b"n_images"), ({"k": 0}, b"k must be"), ({"mode": 2}, b"mode"),
                     ({"mode": -1}, b"mode"), ({"offsets": (1, 3, 8)}, b"offsets[0]"),
                     ({"offsets": (0, 5, 3)}, b"offsets decrease at photograph 1"),
                     ({"offsets": (0, 1025), "n_images": 1}, b"1025"),
                     ({"offsets": (0, 3, 3)}, b"NULL handle"),           # a photograph without a face is legal
                     ({"offsets": (0, 0, 0), "idx": None, "score": None, "out_face": None, "out_score": None},
                      b"NULL handle")):                                  # no face at all: nothing to point at
        rc, msg = call(**kw)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, kw
        assert text in msg, (kw, msg)
    assert not any(out_face) and not any(out_score) and not any(out_image)  # nothing was written
    assert call(n_images=0, offsets=None)[1] == b"NULL handle"


def test_photo_rollcall_op_shapes_without_gpu():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        f, s, im = torch.ops.frhip.photo_rollcall(torch.empty(9, 3, dtype=torch.int32),
                                                  torch.empty(9, 3, dtype=torch.float32), [0, 4, 4, 9], 0.35, 1)
    assert f.shape == (9, 4) and f.dtype == torch.int32 and s.shape == (9,) and s.dtype == torch.float32
    assert im.shape == (3, 4) and im.dtype == torch.int32


def test_planted_situations(host):
    c = CASES["one_row_k1"]
    face, fscore, image = host(c["idx"], c["score"], c["offsets"], 0.35, RC.EXCLUSIVE)
    assert image.tolist() == [[70, 1, 0, 69]] and face[int(np.argmax(c["score"][:, 0])), 0] == RC.RECOGNIZED
    c = CASES["one_row_k1_tied"]
    face = host(c["idx"], c["score"], c["offsets"], 0.35, RC.EXCLUSIVE)[0]
    assert face[0].tolist() == [RC.RECOGNIZED, 7, 0, 0] and (face[1:, 0] == RC.DISPLACED).all()
    c = CASES["chain_50"]
    face, fscore, image = host(c["idx"], c["score"], c["offsets"], 0.35, RC.EXCLUSIVE)
    assert image.tolist() == [[51, 51, 0, 0]]  # every face of the chain is pushed to its second row
    assert face[0, 1:3].tolist() == [1, 0] and np.array_equal(face[1:, 1], np.arange(2, 52))
    assert (face[1:, 2] == 1).all()
    assert host(c["idx"], c["score"], c["offsets"], 0.35, RC.INDEPENDENT)[2].tolist() == [[51, 51, 0, 0]]
    c = CASES["ties_across_faces"]
    face = host(c["idx"], c["score"], c["offsets"], 0.35, RC.EXCLUSIVE)[0]
    # 0.5 everywhere: face 0 takes row 5, face 1 row 6 (its column 1), face 3 row 7 (column 2), face 4 row 8
    assert face.tolist() == [[0, 5, 0, 0], [0, 6, 1, 0], [2, 5, 0, 0], [0, 7, 2, 0], [0, 8, 0, 0]]
    c = CASES["nan_column0"]
    face = host(c["idx"], c["score"], c["offsets"], 0.35, RC.EXCLUSIVE)[0]
    # face 0's top-1 is a NaN; its 0.8 on row 10 loses to face 1's 0.9, its 0.7 on row 11 is granted
    assert face.tolist() == [[0, 11, 2, 0], [0, 10, 0, 0], [RC.CANDIDATE, 13, 0, 0], [0, 9, 0, 0]]
    assert host(c["idx"], c["score"], c["offsets"], 0.35, RC.INDEPENDENT)[0][:, 0].tolist() == [1, 0, 1, 0]
    c = CASES["all_below"]
    for mode in (RC.INDEPENDENT, RC.EXCLUSIVE):
        assert host(c["idx"], c["score"], c["offsets"], -0.2, mode)[2].tolist() == [[3, 0, 3, 0]]
        assert host(c["idx"], c["score"], c["offsets"], -0.25, mode)[2].tolist() == [[3, 1, 2, 0]]
    with pytest.raises(ValueError):
        host(c["idx"], c["score"], c["offsets"], 0.35, 2)
