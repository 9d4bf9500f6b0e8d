"""The letterbox / resize kernels alone, on planted sizes (csrc/detect.hip; host tables in
csrc/detector.cpp, the embedder's table cache in csrc/embed_forward.cpp).

``letterbox_kernel``, ``letterbox_images_kernel`` (through ``frt_letterbox`` / ``frt_letterbox_images``,
on a canvas of any size) and the 112 x 112 crop resize (``fr_resize_crops`` / ``fr_resize_images``) are
held bit for bit to ``oracle.scrfd.letterbox`` / ``resize_linear_u8``.  Sizes are chosen for what the
kernels branch on: every residue of the SSE2 / scalar rounding split (``simd_end``), 4-byte store
groups that are part image and part padding, 1-pixel axes, the exact-2x resize, canvases with and
without padding, the side limit, and more source sizes than the embedder's table cache holds.
``new_w`` / ``new_h`` always come from ``oracle.scrfd.letterbox_geometry``.  Sources hold no zero byte,
so padding is never mistaken for pixels; outputs are pre-filled with 0xA5.

The detector's own per-size table cache (fr_detect_device) needs a whole-network run per size and is
not covered here.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import scrfd as R

FILL = 0xA5

# (dw, dh) -> source sizes (h, w)
BIG = [(128, w) for w in range(1, 17)] + [(1, 640), (2, 3), (3, 2), (1, 1), (1280, 1280), (641, 640), (640, 641)]
CANVASES = {(640, 640): BIG, (640, 448): [(90, 160), (9, 16)]}  # 448 rows: a row-reduced canvas, 360 rows of content
for _dw, _dh in itertools.product((4, 8, 12, 20), (1, 3, 16)):
    CANVASES[(_dw, _dh)] = [(3 * _dh + 1, 1), (3 * _dh + 1, 2), (3 * _dh + 1, 3), (5 * _dh, 4), (_dh, _dw),
                            (2 * _dh, 2 * _dw), (1, _dw), (7, 5), (2, 3)]
CANVASES[(16, 16)] = [(32, 32), (16, 16), (33, 7)]
THREE_FRAMES = {(640, 640): (2, 3), (16, 16): (32, 32), (8, 16): (7, 5)}  # canvases whose one-size launch of this source has n = 3


def _geometry(dw, dh):
    """[(h, w, new_w, new_h)] of the canvas's sources the letterbox takes (both new sides >= 1)."""
    out = []
    for h, w in dict.fromkeys(CANVASES[(dw, dh)]):
        new_w, new_h, _ = R.letterbox_geometry(h, w, dw, dh)
        if new_w >= 1 and new_h >= 1:
            assert new_w <= dw and new_h <= dh
            out.append((h, w, new_w, new_h))
    return out


def _img(h, w, seed=0):
    return np.random.default_rng(h * 10007 + w + 7919 * seed).integers(1, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(dw, dh, h, w, seed=0):
    ref = R.letterbox(_img(h, w, seed), dw, dh)[0]
    ref.setflags(write=False)
    return ref


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_planted_sizes_cover_what_the_kernels_branch_on():
    """No kernel runs: the geometry the cases below rely on."""
    from tests import _frt
    big = _geometry(640, 640)
    assert [g[2:] for g in big[:16]] == [(5 * w, 640) for w in range(1, 17)]
    assert {g[2] % 16 for g in big[:16]} == set(range(16)) and {g[2] * 3 % 4 for g in big[:16]} == {0, 1, 2, 3}
    ends = {_frt.resize_simd_end(g[2] * 3) for g in big[:16]}
    assert len(ends) >= 12 and all(e % 8 == 0 for e in ends)       # a different split nearly every width
    assert big[16][2:] == (640, 1) and big[19][2:] == (640, 640) and big[20][2:] == (640, 640)
    assert big[21][2:] == (639, 640) and big[22][2:] == (640, 639)
    assert _geometry(640, 448)[0][2:] == (640, 360)
    small = [(dw, dh) + g for (dw, dh) in CANVASES if dw <= 20 for g in _geometry(dw, dh)]
    assert {g[4] * 3 % 4 for g in small if g[4] < g[0]} == {0, 1, 2, 3}   # store groups part image, part padding
    assert any(g[4] == g[0] and g[5] == g[1] for g in small)              # no padding at all
    assert any(g[1] == 16 and g[5] == 1 for g in small)                   # one row of content on 16
    assert (16, 16, 32, 32, 16, 16) in small                              # the exact-2x resize
    assert {g[0] for g in small} == {4, 8, 12, 16, 20} and {g[1] for g in small} == {1, 3, 16}


@pytest.mark.gpu
@pytest.mark.parametrize("dw,dh", list(CANVASES), ids=lambda v: str(v))
def test_letterbox_kernels_alone(dw, dh):
    from tests import _frt
    geo = _geometry(dw, dh)
    assert len(geo) >= 2
    canvas = dh * dw * 3
    one_size = []
    for h, w, new_w, new_h in geo:
        n = 3 if THREE_FRAMES.get((dw, dh)) == (h, w) else 1
        frames = np.stack([_img(h, w, s) for s in range(n)])
        out = torch.full((n * canvas + 64,), FILL, dtype=torch.uint8, device="cuda")
        _frt.letterbox(_dev(frames), new_w, new_h, dw, dh, out)
        got = out.cpu().numpy()
        assert (got[n * canvas:] == FILL).all(), f"{h}x{w}: bytes after the last canvas were written"
        got = got[:n * canvas].reshape(n, dh, dw, 3)
        for s in range(n):
            ref = _reference(dw, dh, h, w, s)
            assert np.array_equal(got[s], ref), f"{h}x{w} frame {s}: {np.count_nonzero(got[s] != ref)} bytes differ"
        assert not got[0, new_h:].any() and not got[0, :, new_w:].any() and got[0, :new_h, :new_w].all()
        one_size.append(got[0])
    # the ragged kernel: the whole list in one launch, shuffled
    order = np.random.default_rng(dw * 1000 + dh).permutation(len(geo))
    images = [_dev(_img(*geo[i][:2])) for i in order]
    out = torch.full((len(geo) * canvas + 64,), FILL, dtype=torch.uint8, device="cuda")
    _frt.letterbox_images(images, [(geo[i][3], geo[i][2]) for i in order], dw, dh, out)
    got = out.cpu().numpy()
    assert (got[len(geo) * canvas:] == FILL).all()
    got = got[:len(geo) * canvas].reshape(len(geo), dh, dw, 3)
    for k, i in enumerate(order):
        assert np.array_equal(got[k], one_size[i]), f"ragged image {k} ({geo[i][0]}x{geo[i][1]}) != the one-size kernel"


@pytest.mark.gpu
def test_letterbox_entries_refuse_what_the_launchers_refuse():
    from tests import _frt
    src = _dev(_img(7, 5))
    out = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    bad = [dict(new_w=3, new_h=4, dw=6, dh=8, out=out),        # dw * 3 % 4 != 0
           dict(new_w=5, new_h=7, dw=8, dh=8, out=out[1:]),    # misaligned out
           dict(new_w=9, new_h=7, dw=8, dh=8, out=out),        # new_w > dw
           dict(new_w=5, new_h=9, dw=8, dh=8, out=out),        # new_h > dh
           dict(new_w=0, new_h=7, dw=8, dh=8, out=out)]
    for kw in bad:
        with pytest.raises(ValueError):
            _frt.letterbox(src[None], **kw)
        with pytest.raises(ValueError):
            _frt.letterbox_images([src], [(kw["new_h"], kw["new_w"])], kw["dw"], kw["dh"], kw["out"])
    torch.cuda.synchronize()
    assert (out == FILL).all()


# ------------------------------------------------------------------ fr_resize_crops / fr_resize_images
CROP_SIZES = [(1, 1), (1, 300), (300, 1), (2, 2), (56, 56), (111, 113), (113, 112), (223, 225), (8192, 1), (1, 8192)]
CACHE_SIZES = [(3 + i, 40 - 2 * i) for i in range(17)]  # 17 distinct sizes: one more than the handle's table cache


def _handle(max_batch=4):
    from facerecognitionpipeline_amd import _lib
    return _lib.Handle("ir_50", "adaface", torch.device("cuda", 0), max_batch=max_batch)  # never finalised


@functools.lru_cache(maxsize=None)
def _crop_reference(h, w, seed=0):
    ref = R.resize_linear_u8(_img(h, w, seed), 112, 112)
    ref.setflags(write=False)
    return ref


def _resize_crop(handle, h, w, seed=0):
    out = torch.full((1, 112, 112, 3), FILL, dtype=torch.uint8, device="cuda")
    handle.resize_crops(_dev(_img(h, w, seed)[None]), out)
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


@pytest.fixture(scope="module")
def crops_handle():
    h = _handle()
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", CROP_SIZES)
def test_resize_crops_planted_sizes(crops_handle, h, w):
    got = _resize_crop(crops_handle, h, w)
    ref = _crop_reference(h, w)
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(8193, 1), (1, 8193), (0, 5)])
def test_resize_crops_refuses_sides_out_of_range(crops_handle, h, w):
    out = torch.full((1, 112, 112, 3), FILL, dtype=torch.uint8, device="cuda")
    src = torch.full((1, h, w, 3), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        crops_handle.resize_crops(src, out)
    torch.cuda.synchronize()
    assert (out == FILL).all()


@pytest.mark.gpu
def test_resize_table_cache_replaces_and_never_serves_a_stale_table():
    """17 sizes through a fresh handle's 16-entry table cache: the 17th replaces the least recently
    used table (the first size's), the first size again replaces the second's, and the reverse pass
    hits and replaces in the other order.  A stale or mis-keyed table shows as wrong pixels."""
    assert len(set(CACHE_SIZES)) == 17
    h = _handle()
    try:
        for hw in CACHE_SIZES + CACHE_SIZES[:1] + CACHE_SIZES[::-1]:
            got = _resize_crop(h, *hw)
            assert np.array_equal(got, _crop_reference(*hw)), f"{hw}: {np.count_nonzero(got != _crop_reference(*hw))}"
        # the same sizes as one ragged list: chunks of max_batch = 4, a size twice in a chunk
        sizes = CACHE_SIZES[:2] + [CACHE_SIZES[0]] + CACHE_SIZES[2:] + [CACHE_SIZES[16], CACHE_SIZES[3]]
        seeds = [0, 0, 1] + [0] * 15 + [1, 1]
        out = torch.full((len(sizes), 112, 112, 3), FILL, dtype=torch.uint8, device="cuda")
        h.resize_images([_dev(_img(a, b, s)) for (a, b), s in zip(sizes, seeds)], out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i, ((a, b), s) in enumerate(zip(sizes, seeds)):
            assert np.array_equal(got[i], _crop_reference(a, b, s)), f"image {i} ({a}x{b})"
            if s == 0:
                assert np.array_equal(got[i], _resize_crop(h, a, b))
    finally:
        h.close()
