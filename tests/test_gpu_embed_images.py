"""Mixed-size crop lists: ``fr_resize_images`` / ``fr_embed_images`` (one call that resizes / embeds n
crops of n sizes, one staging copy and one launch per ``max_batch`` chunk) and
``FaceEmbedder.embed_images`` on them.

Per crop the resize is ``fr_resize_crops`` of that crop alone, bit for bit (and OpenCV's fixed-point
INTER_LINEAR as ``oracle.scrfd.resize_linear_u8`` restates it); the embedding is ``fr_embed`` of the
resized list, bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import scrfd as R

pytestmark = pytest.mark.gpu

EMB_TOL = 1e-5  # the project's embedding tolerance (tests/test_gpu_pipeline.py)
# exact 2x, identity, one pixel, off by one both ways, a size repeated inside a chunk, upscaling, one
# identity axis, an extreme aspect, and a chunk of one image (max_batch 4: chunks 4 / 4 / 1)
SIZES = [(224, 224), (112, 112), (1, 1), (113, 111), (224, 224), (96, 96), (112, 200), (300, 7), (480, 640)]
MAX_BATCH = 4
MARK = 0xA5


@pytest.fixture(scope="module")
def emb():
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    return FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=MAX_BATCH)


@pytest.fixture(scope="module")
def crops():
    r = np.random.Generator(np.random.PCG64(0xFACE0112))
    return [r.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SIZES]


@pytest.fixture(scope="module")
def dev_crops(emb, crops):
    return [torch.from_numpy(c).to(emb.device) for c in crops]


@pytest.fixture(scope="module")
def resized(emb, dev_crops):
    out = torch.full((len(SIZES), 112, 112, 3), MARK, dtype=torch.uint8, device=emb.device)
    emb.model.resize_images(dev_crops, out)
    torch.cuda.synchronize()
    return out


def test_resize_is_the_oracle(crops, resized):
    got = resized.cpu().numpy()
    for i, c in enumerate(crops):
        assert np.array_equal(got[i], R.resize_linear_u8(c, 112, 112)), SIZES[i]


def test_resize_is_resize_crops_of_each_crop_alone(emb, dev_crops, resized):
    for i, c in enumerate(dev_crops):
        one = torch.empty((1, 112, 112, 3), dtype=torch.uint8, device=emb.device)
        emb.model.resize_crops(c[None].contiguous(), one)
        assert torch.equal(one[0], resized[i]), SIZES[i]


def test_identity_size_comes_through(crops, resized):
    assert np.array_equal(resized[1].cpu().numpy(), crops[1])
    # (an address that rules the 4-byte copy out takes the table path to the same bytes)
    flat = torch.zeros(112 * 112 * 3 + 1, dtype=torch.uint8, device=resized.device)
    flat[1:] = torch.from_numpy(crops[1]).to(resized.device).reshape(-1)
    view = flat[1:].view(112, 112, 3)
    assert view.data_ptr() % 4 == 1
    from facerecognitionpipeline_amd.torch_ops import utility_handle
    out = torch.empty((1, 112, 112, 3), dtype=torch.uint8, device=resized.device)
    utility_handle(resized.device).resize_images([view], out)
    assert np.array_equal(out[0].cpu().numpy(), crops[1])


def test_resize_on_an_unfinalised_handle(emb, dev_crops, resized):
    from facerecognitionpipeline_amd import _lib
    h = _lib.Handle("ir_50", "adaface", emb.device, max_batch=MAX_BATCH)  # no weights loaded
    try:
        out = torch.empty_like(resized)
        h.resize_images(dev_crops, out)
        assert torch.equal(out, resized)
        with pytest.raises(_lib.FrHipError, match="not finalised"):
            h.embed_images(dev_crops, torch.empty((len(SIZES), 512), dtype=torch.float32, device=emb.device))
    finally:
        h.close()


@pytest.fixture(scope="module")
def embedded(emb, dev_crops):
    return {norm: emb.embed_images(dev_crops, normalize=norm) for norm in (True, False)}


@pytest.mark.parametrize("normalize", [True, False])
def test_embed_is_embed_tensor_of_the_resized_list(emb, resized, embedded, normalize):
    want = emb.embed_tensor(resized, normalize=normalize)
    assert torch.equal(embedded[normalize], want)


def test_embed_matches_the_per_size_path(emb, crops, embedded):
    want = emb.extract_embeddings_batch(crops, normalize=True)
    err = np.abs(embedded[True].cpu().numpy() - want).max()
    print("embed_images vs extract_embeddings_batch: max abs diff", err)
    assert err <= EMB_TOL


def test_embed_host_arrays_and_twice(emb, crops, embedded):
    again = emb.embed_images(crops, normalize=True)  # host arrays: one packed upload
    assert torch.equal(again, embedded[True])
    mixed = emb.embed_images([c if i % 2 else torch.from_numpy(c).to(emb.device) for i, c in enumerate(crops)])
    assert torch.equal(mixed, embedded[True])


def test_embed_small_list_and_chunk_for_chunk(emb, crops, resized, embedded):
    """Three crops of one size (below graph_batch).  Their rows are NOT bitwise rows 0 and 4 of the
    9-crop run (seen on an MI355X: 1.2e-7 at most in a component): there they ran in
    forwards of four crops, here in a forward of three, and the forward picks its kernels and split-K
    factors by the batch it runs -- a property of the forward's batch size, not of graph replay and
    not of this call.  So: the first call (eager, then captured) and the second (replayed) give the
    same bits, they are ``embed_tensor``'s bits for the same three resized crops, and the 9-crop
    run is compared chunk for chunk: a list that is one of its chunks gives that chunk's bits."""
    r = np.random.Generator(np.random.PCG64(0xFACE0113))
    three = [crops[0], crops[4], r.integers(0, 256, size=(224, 224, 3), dtype=np.uint8)]
    first = emb.embed_images(three)
    assert torch.equal(emb.embed_images(three), first)
    small = torch.empty((3, 112, 112, 3), dtype=torch.uint8, device=emb.device)
    emb.model.resize_images([torch.from_numpy(c).to(emb.device) for c in three], small)
    assert torch.equal(small[:2], resized[[0, 4]])
    assert torch.equal(first, emb.embed_tensor(small))
    diff = (first[:2] - embedded[True][[0, 4]]).abs().max().item()
    print("3-crop forward vs the same crops in 4-crop forwards: max abs diff", diff)
    assert diff <= EMB_TOL
    for lo, hi in ((0, 4), (4, 8), (8, 9)):
        assert torch.equal(emb.embed_images(crops[lo:hi]), embedded[True][lo:hi]), (lo, hi)


def _raw_call(emb, fn, ptrs, sizes, out, *tail):
    p = np.asarray(ptrs, dtype=np.uint64)
    s = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
    return getattr(emb.model._lib, fn)(emb.model.h, p.ctypes.data, s.ctypes.data, len(p), out.data_ptr(), *tail,
                                       torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("what", ["null", "side_0", "side_8193"])
@pytest.mark.parametrize("fn", ["fr_resize_images", "fr_embed_images"])
def test_a_refused_image_is_named_and_nothing_runs(emb, dev_crops, fn, what):
    from facerecognitionpipeline_amd import _lib
    ptrs = [c.data_ptr() for c in dev_crops]
    sizes = [list(s) for s in SIZES]
    if what == "null":
        ptrs[5] = 0
    elif what == "side_0":
        sizes[5][1] = 0
    else:
        sizes[5][0] = 8193
    if fn == "fr_resize_images":
        out = torch.full((len(SIZES), 112, 112, 3), MARK, dtype=torch.uint8, device=emb.device)
        tail = ()
    else:
        out = torch.full((len(SIZES), 512), float(MARK), dtype=torch.float32, device=emb.device)
        tail = (1,)
    rc = _raw_call(emb, fn, ptrs, sizes, out, *tail)
    assert rc == _lib.FR_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match=r"image 5\b"):
        _lib.check(rc, emb.model.h)
    torch.cuda.synchronize()
    assert bool((out == MARK).all())


def test_null_arrays_and_empty_list(emb, dev_crops):
    from facerecognitionpipeline_amd import _lib
    L, h, s = emb.model._lib, emb.model.h, torch.cuda.current_stream().cuda_stream
    out = torch.empty((1, 112, 112, 3), dtype=torch.uint8, device=emb.device)
    sizes = np.array([[224, 224]], np.int32)
    ptrs = np.array([dev_crops[0].data_ptr()], np.uint64)
    assert L.fr_resize_images(h, None, sizes.ctypes.data, 1, out.data_ptr(), s) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_resize_images(h, ptrs.ctypes.data, None, 1, out.data_ptr(), s) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_resize_images(h, ptrs.ctypes.data, sizes.ctypes.data, 1, None, s) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_embed_images(h, None, None, 1, None, 1, s) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_resize_images(h, None, None, 0, None, s) == _lib.FR_OK
    assert L.fr_embed_images(h, None, None, 0, None, 1, s) == _lib.FR_OK
    assert tuple(emb.embed_images([]).shape) == (0, 512)
    emb.model.resize_images([], torch.empty((0, 112, 112, 3), dtype=torch.uint8, device=emb.device))
