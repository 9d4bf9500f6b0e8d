"""ctypes binding of include/frhip_testing.h (kernel-level test entry points)."""
import ctypes

import torch

from facerecognitionpipeline_amd import _lib

_P = ctypes.c_void_p
_I = ctypes.c_int


def lib():
    L = _lib.load()
    if not getattr(L, "_frt_ready", False):
        L.frt_conv2d.restype = _I
        L.frt_conv2d.argtypes = [_P, _P, _P] + [_I] * 9 + [_P] * 6 + [_I] * 7 + [_P]
        L.frt_conv2d_fused.restype = _I
        L.frt_conv2d_fused.argtypes = [_P, _P, _P, _P] + [_I] * 10 + [_P] * 6 + [_I] * 7 + [_P]
        L.frt_conv_split_fixup.restype = _I
        L.frt_conv_split_fixup.argtypes = [_P, _I, ctypes.c_longlong] + [_I] * 4 + [_P] * 3 + [_I] * 3 + [_P, _P]
        L.frt_conv2d_winograd.restype = _I
        L.frt_conv2d_winograd.argtypes = [_P, _P, _P] + [_I] * 5 + [_P] * 6 + [_I, _P]
        L.frt_conv2d_winograd4_ex.restype = _I
        L.frt_conv2d_winograd4_ex.argtypes = [_P, _P, _P] + [_I] * 5 + [_P] * 6 + [_I, _I, _P]
        L.frt_set_wino4_split.restype = _I
        L.frt_set_wino4_split.argtypes = [_I]
        L.frt_set_conv2sc_tile.restype = _I
        L.frt_set_conv2sc_tile.argtypes = [_I]
        L.frt_maxpool3.restype = _I
        L.frt_maxpool3.argtypes = [_P, _I, _I, _I, _I, _P, _P]
        L.frt_set_wino4_nbg.restype = _I
        L.frt_set_wino4_nbg.argtypes = [_I]
        L.frt_set_wino4_shapes.restype = _I
        L.frt_set_wino4_shapes.argtypes = [_I]
        L.frt_set_wino4_max_split.restype = _I
        L.frt_set_wino4_max_split.argtypes = [_I]
        L.frt_set_wino4_poll_limit.restype = _I
        L.frt_set_wino4_poll_limit.argtypes = [_I]
        L.frt_set_s2_band.restype = _I
        L.frt_set_s2_band.argtypes = [_I]
        L.frt_conv2d_s2band.restype = _I
        L.frt_conv2d_s2band.argtypes = [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P]
        L.frt_set_fuse_shortcut.restype = _I
        L.frt_set_fuse_shortcut.argtypes = [_P, _I]
        L.frt_set_small_conv.restype = _I
        L.frt_set_small_conv.argtypes = [_P, _I]
        L.frt_set_small_conv_pre_epilogue.restype = _I
        L.frt_set_small_conv_pre_epilogue.argtypes = [_P, _I]
        L.frt_set_small_conv_blocked.restype = _I
        L.frt_set_small_conv_blocked.argtypes = [_P, _I]
        L.frt_set_small_conv_pixels.restype = _I
        L.frt_set_small_conv_pixels.argtypes = [_P, _I]
        L.frt_set_wino4_blocked.restype = _I
        L.frt_set_wino4_blocked.argtypes = [_P, _I]
        L.frt_conv2d_small_ex.restype = _I
        L.frt_conv2d_small_ex.argtypes = [_P, _P, _P, _P] + [_I] * 7 + [_P] * 6 + [_I, _I, _P, _P, _P, _P]
        L.frt_head_reduce.restype = _I
        L.frt_head_reduce.argtypes = [_P, _I, ctypes.c_longlong, _P, _P, _P, _P, _I, _I, _I, _P]
        L.frt_stem.restype = _I
        L.frt_stem.argtypes = [_P, _I, _P, _P, _P, _P, _P, _P, _P]
        L.frt_topk.restype = _I
        L.frt_topk.argtypes = [_P, _I, _I, _I, _P, _P, _P]
        L.frt_topk_ex.restype = _I
        L.frt_topk_ex.argtypes = [_P, _I, _I, _I, _I, _P, _P, _P]
        L.frt_detector_forward.restype = _I
        L.frt_detector_forward.argtypes = [_P, _P, _I, _I, _I, _P, _P, _P]
        L.frt_set_detector_row_reduction.restype = _I
        L.frt_set_detector_row_reduction.argtypes = [_P, _I]
        L.frt_upsample_add.restype = _I
        L.frt_upsample_add.argtypes = [_P, _P, _I, _I, _I, _I, _P]
        L.frt_avgpool2.restype = _I
        L.frt_avgpool2.argtypes = [_P, _I, _I, _I, _I, _P, _P]
        L.frt_row_expand.restype = _I
        L.frt_row_expand.argtypes = [_P, _I, _I, _I, _I, _I, _I, _P, _P]
        L.frt_det_stem.restype = _I
        L.frt_det_stem.argtypes = [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]
        L.frt_detector_postprocess.restype = _I
        L.frt_detector_postprocess.argtypes = [_P, _P, _I, ctypes.c_float, _P, ctypes.c_float, _I, _P, _P, _P]
        L.frt_warp_affine_images.restype = _I
        L.frt_warp_affine_images.argtypes = [_P, _P, _I, _P, _P, _I, _I, _P, _P]
        L.frt_letterbox.restype = _I
        L.frt_letterbox.argtypes = [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]
        L.frt_letterbox_images.restype = _I
        L.frt_letterbox_images.argtypes = [_P, _P, _P, _I, _I, _I, _P, _P]
        L.frt_resize_simd_end.restype = _I
        L.frt_resize_simd_end.argtypes = [_I]
        L._frt_ready = True
    return L


def _image_arrays(images):
    """A list of contiguous uint8 [H,W,3] cuda tensors -> (host pointer array uint64 [n], sizes int32 [n,2])."""
    import numpy as np
    for im in images:
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous() and im.is_cuda
    ptrs = np.array([im.data_ptr() for im in images], dtype=np.uint64)
    sizes = np.array([[im.shape[0], im.shape[1]] for im in images], dtype=np.int32).reshape(-1, 2)
    return ptrs, sizes


def warp_affine_images(images, face_image, tforms, out_size, out=None):
    """The ragged warp kernel on caller-supplied forward maps: images a list of uint8 [H,W,3] cuda
    tensors, face_image int [n], tforms float64 [n,2,3] -> uint8 [n,S,S,3] (pre-filled with 0xA5, or
    the caller's `out`)."""
    import numpy as np
    ptrs, sizes = _image_arrays(images)
    fi = np.ascontiguousarray(face_image, dtype=np.int32).reshape(-1)
    tf = np.ascontiguousarray(tforms, dtype=np.float64).reshape(-1, 2, 3)
    n, S = fi.shape[0], int(out_size)
    assert tf.shape[0] == n
    if out is None:
        out = torch.full((n, max(S, 0), max(S, 0), 3), 0xA5, dtype=torch.uint8, device=images[0].device)
    _lib.check(lib().frt_warp_affine_images(ptrs.ctypes.data, sizes.ctypes.data, len(images), fi.ctypes.data,
                                            tf.ctypes.data, n, S, _p(out), torch.cuda.current_stream().cuda_stream))
    return out


def letterbox(frames, new_w, new_h, dw, dh, out):
    """letterbox_kernel alone: frames uint8 [n,H,W,3] cuda -> the first n canvases of `out` (uint8 cuda,
    at least n * dh * dw * 3 bytes, written in place so a test sees what lies behind them)."""
    n, H, W = frames.shape[:3]
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and out.dtype == torch.uint8
    assert dw < 1 or dh < 1 or out.numel() >= n * dh * dw * 3
    _lib.check(lib().frt_letterbox(_p(frames), n, H, W, int(new_w), int(new_h), int(dw), int(dh), _p(out),
                                   torch.cuda.current_stream().cuda_stream))
    return out


def letterbox_images(images, new_sizes, dw, dh, out):
    """letterbox_images_kernel alone: images a list of uint8 [H,W,3] cuda tensors, new_sizes [(new_h,
    new_w)] per image -> the first len(images) canvases of `out`."""
    import numpy as np
    ptrs, sizes = _image_arrays(images)
    ns = np.ascontiguousarray(new_sizes, dtype=np.int32).reshape(-1, 2)
    assert ns.shape[0] == len(images) and out.dtype == torch.uint8
    assert dw < 1 or dh < 1 or out.numel() >= len(images) * dh * dw * 3
    _lib.check(lib().frt_letterbox_images(ptrs.ctypes.data, sizes.ctypes.data, ns.ctypes.data, len(images), int(dw),
                                          int(dh), _p(out), torch.cuda.current_stream().cuda_stream))
    return out


def resize_simd_end(row_elems):
    """The host's split between SSE2 and scalar vertical rounding of a resized row (no GPU needed)."""
    return int(lib().frt_resize_simd_end(int(row_elems)))


def _p(t):
    return None if t is None else t.data_ptr()


def _conv_out(x, B, H, W, cout, kh, kw, stride, pad, nsplit, out):
    """The NaN-filled output of a conv wrapper, or the caller's `out` of that shape (a test of a
    refusal passes its own, to see after the raise that nothing was written)."""
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    if out is None:
        return torch.full((nsplit, B, Ho, Wo, cout), float("nan"), device=x.device)
    assert out.shape == (nsplit, B, Ho, Wo, cout) and out.dtype == torch.float32 and out.is_contiguous()
    return out


def conv2d(x, w, B, H, W, cin, cout, kh, kw, stride, pad, pre=None, post=None, prelu=None, res=None,
           res_hw=(0, 0), epi=0, nsplit=1, tile=1, stream_k=0, precision=0, out=None):
    """x: NHWC cuda f32, w: [cout][kh][kw][cin] cuda f32.  Returns y (NHWC) or partial slabs."""
    y = _conv_out(x, B, H, W, cout, kh, kw, stride, pad, nsplit, out)
    ps, ph = (pre if pre is not None else (None, None))
    qs, qh = (post if post is not None else (None, None))
    rc = lib().frt_conv2d(_p(x), _p(w), _p(y), B, H, W, cin, cout, kh, kw, stride, pad, _p(ps), _p(ph), _p(qs),
                          _p(qh), _p(prelu), _p(res), res_hw[0], res_hw[1], epi, nsplit, tile, stream_k, precision,
                          torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return y if nsplit > 1 else y[0]


def conv2d_fused(x, x2, w, B, H, W, cin, cin2, cout, kh, kw, stride, pad, pre=None, post=None, prelu=None, res=None,
                 res_hw=(0, 0), epi=0, nsplit=1, tile=1, stream_k=0, precision=0, out=None):
    """The MFMA kernel with its fused 1x1 shortcut: x NHWC [B,H,W,cin], x2 NHWC [B,H,W,cin2] (read at the
    output's stride), w [cout][kh*kw*cin + cin2] cuda f32.  Returns y (NHWC) or partial slabs."""
    y = _conv_out(x, B, H, W, cout, kh, kw, stride, pad, nsplit, out)
    ps, ph = (pre if pre is not None else (None, None))
    qs, qh = (post if post is not None else (None, None))
    rc = lib().frt_conv2d_fused(_p(x), _p(x2), _p(w), _p(y), B, H, W, cin, cin2, cout, kh, kw, stride, pad, _p(ps),
                                _p(ph), _p(qs), _p(qh), _p(prelu), _p(res), res_hw[0], res_hw[1], epi, nsplit, tile,
                                stream_k, precision, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return y if nsplit > 1 else y[0]


def conv_split_fixup(part, S, stride, B, Ho, Wo, cout, post, res=None, res_hw=(0, 0), epi=0, out=None):
    """conv_split_fixup_kernel alone: part cuda f32 holding S slabs `stride` floats apart -> y [B,Ho,Wo,cout]."""
    y = torch.full((B, Ho, Wo, cout), float("nan"), device=part.device) if out is None else out
    assert y.shape == (B, Ho, Wo, cout) and y.dtype == torch.float32 and y.is_contiguous()
    rc = lib().frt_conv_split_fixup(_p(part), S, stride, B, Ho, Wo, cout, _p(post[0]), _p(post[1]), _p(res),
                                    res_hw[0], res_hw[1], epi, _p(y), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return y


W4_BLK_X, W4_BLK_RES, W4_BLK_Y = 1, 2, 4
CONVS_BLK_X, CONVS_BLK_X2, CONVS_BLK_RES, CONVS_BLK_Y = 1, 2, 4, 8


def to_blocked(nhwc):
    """[B][H][W][C] -> the channel-blocked [B][C/16][H][W][16] (contiguous)."""
    B, H, W, C = nhwc.shape
    return nhwc.view(B, H, W, C // 16, 16).permute(0, 3, 1, 2, 4).contiguous()


def from_blocked(t):
    """[B][C/16][H][W][16] -> NHWC [B][H][W][C] (contiguous)."""
    B, CB, H, W, _ = t.shape
    return t.permute(0, 2, 3, 1, 4).contiguous().view(B, H, W, CB * 16)


def _as(t, blocked):
    """A wrapper's NHWC input in the layout the launch reads it in."""
    return t if t is None or not blocked else to_blocked(t)


def _unblock(y, blocked):
    """A wrapper's output buffer (allocated in the NHWC shape; the blocked layout has the same float
    count, so every element of it is written too) back in NHWC."""
    if not blocked:
        return y
    B, H, W, C = y.shape
    return from_blocked(y.view(B, C // 16, H, W, 16))


def conv2d_winograd(x, w, B, H, W, cin, cout, pre=None, post=None, prelu=None, res=None, epi=1, m=2, blk=0, out=None):
    """Winograd F(mxm,3x3) stride-1 conv (m = 2 or 4);
    x NHWC cuda f32, w [cout][3][3][cin] cuda f32.  blk (m = 4): the W4_BLK_* tensors are handed to
    the kernel channel-blocked (x and res are blocked here, y is unblocked here: NHWC in and out).
    out: the caller's buffer instead of a fresh NaN-filled one (returned as the kernel left it)."""
    y = torch.full((B, H, W, cout), float("nan"), device=x.device) if out is None else out
    assert y.shape == (B, H, W, cout) and y.dtype == torch.float32 and y.is_contiguous()
    ps, ph = (pre if pre is not None else (None, None))
    qs, qh = post
    x, res = _as(x, blk & W4_BLK_X), _as(res, blk & W4_BLK_RES)
    if m == 4:
        rc = lib().frt_conv2d_winograd4_ex(_p(x), _p(w), _p(y), B, H, W, cin, cout, _p(ps), _p(ph), _p(qs), _p(qh),
                                           _p(prelu), _p(res), epi, blk, torch.cuda.current_stream().cuda_stream)
    else:
        assert blk == 0
        rc = lib().frt_conv2d_winograd(_p(x), _p(w), _p(y), B, H, W, cin, cout, _p(ps), _p(ph), _p(qs), _p(qh),
                                       _p(prelu), _p(res), epi, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return y if out is not None else _unblock(y, blk & W4_BLK_Y)


def head_reduce(partial, nsplit, split_stride, fc_bias, bn_scale, bn_shift, n, normalize, model_l2, out=None):
    """head_reduce_kernel alone: partial cuda f32 holding nsplit slabs `split_stride` floats apart,
    each [n][512] -> emb [n][512] (NaN-filled first, or the caller's `out`)."""
    emb = torch.full((n, 512), float("nan"), device=fc_bias.device) if out is None else out
    rc = lib().frt_head_reduce(_p(partial), nsplit, split_stride, _p(fc_bias), _p(bn_scale), _p(bn_shift), _p(emb), n,
                               int(normalize), int(model_l2), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return emb


def stem(img, lut, w27x64, sc, sh, al):
    B = img.shape[0]
    y = torch.full((B, 112, 112, 64), float("nan"), device=img.device)
    _lib.check(lib().frt_stem(_p(img), B, _p(lut), _p(w27x64), _p(sc), _p(sh), _p(al), _p(y),
                              torch.cuda.current_stream().cuda_stream))
    return y


def maxpool3(x):
    """MaxPool2d(3, 2, 1) of x [B][H][W][C] (NHWC cuda f32) on the detector's kernel."""
    B, H, W, C = x.shape
    y = torch.full((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), float("nan"), device=x.device)
    _lib.check(lib().frt_maxpool3(_p(x), B, H, W, C, _p(y), torch.cuda.current_stream().cuda_stream))
    return y


def upsample_add(big, small):
    """big [B][2h][2w][C] + nearest-2x(small [B][h][w][C]) on the detector's kernel (big is not changed)."""
    B, h, w, C = small.shape
    out = big.clone()
    _lib.check(lib().frt_upsample_add(_p(out), _p(small), B, h, w, C, torch.cuda.current_stream().cuda_stream))
    return out


def avgpool2(x):
    """AvgPool2d(2, 2) of x [B][H][W][C] (NHWC cuda f32) on the detector's kernel."""
    B, H, W, C = x.shape
    y = torch.full((B, H // 2, W // 2, C), float("nan"), device=x.device)
    _lib.check(lib().frt_avgpool2(_p(x), B, H, W, C, _p(y), torch.cuda.current_stream().cuda_stream))
    return y


def row_expand(x, m, Hd):
    """x [B][Hs][W][C] -> [B][Hd][W][C] with row m repeated Hd - Hs more times (row_expand_kernel)."""
    B, Hs, W, C = x.shape
    y = torch.full((B, max(Hd, 0), W, C), float("nan"), device=x.device)
    _lib.check(lib().frt_row_expand(_p(x), B, Hs, W, C, m, Hd, _p(y), torch.cuda.current_stream().cuda_stream))
    return y


def det_stem(img, w27xC, scale, shift, force_scalar=False):
    """The detector stem on img uint8 [B][H][W][3] (cuda), w27xC f32 [27][C]: y [B][H/2][W/2][C]."""
    B, H, W, _ = img.shape
    C = w27xC.shape[1]
    y = torch.full((B, H // 2, W // 2, C), float("nan"), device=img.device)
    _lib.check(lib().frt_det_stem(_p(img), B, H, W, C, _p(w27xC), _p(scale), _p(shift), _p(y), int(force_scalar),
                                  torch.cuda.current_stream().cuda_stream))
    return y


def detector_postprocess(handle, heads, det_scale=1.0, det_scales=None, det_thresh=0.5, max_faces=256):
    """The product's decode + sort + NMS + copy-out on caller-supplied head maps.

    heads: the three levels' maps, numpy f32 [n][hw][32] each.  det_scales: None or n per-frame scales.
    Returns (dets f32 [n][max_faces][15] pre-filled with NaN, so rows the call did not write stay
    visible, counts int32 [n] pre-filled with -1)."""
    import numpy as np
    n = heads[0].shape[0]
    flat = np.concatenate([np.ascontiguousarray(h, dtype=np.float32).reshape(-1) for h in heads])
    dev = torch.from_numpy(flat).to(handle.device)
    dets = np.full((n, max_faces, 15), np.nan, dtype=np.float32)
    counts = np.full(n, -1, dtype=np.int32)
    sc = None
    if det_scales is not None:
        sc = np.ascontiguousarray(det_scales, dtype=np.float32)
        assert sc.shape == (n,)
    rc = lib().frt_detector_postprocess(handle.h, _p(dev), n, float(det_scale), None if sc is None else sc.ctypes.data,
                                        float(det_thresh), int(max_faces), dets.ctypes.data, counts.ctypes.data,
                                        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, handle.h)
    return dets, counts


def topk(scores, k, low_first=False):
    """Row-wise top-k of scores f32 [n][G], read at the tensor's own data pointer (a row-contiguous
    view that starts inside its buffer is taken as it is).  low_first: equal scores by ascending
    index (fr_match_identities' order) instead of descending.  Outputs pre-filled (idx -2, val NaN)."""
    n, G = scores.shape
    assert scores.dtype == torch.float32 and scores.is_contiguous()
    idx = torch.full((n, k), -2, dtype=torch.int32, device=scores.device)
    val = torch.full((n, k), float("nan"), dtype=torch.float32, device=scores.device)
    stream = torch.cuda.current_stream().cuda_stream
    if low_first:
        _lib.check(lib().frt_topk_ex(_p(scores), n, G, k, 1, _p(idx), _p(val), stream))
    else:
        _lib.check(lib().frt_topk(_p(scores), n, G, k, _p(idx), _p(val), stream))
    return idx, val


def detector_forward(handle, frames):
    """Letterbox + SCRFD network on the GPU -> ([3 level maps [n,h,w,32]], canvas [n,640,640,3])."""
    n, H, W = frames.shape[:3]
    sizes = [(640 // s, 640 // s) for s in (8, 16, 32)]
    heads = torch.empty(sum(n * h * w * 32 for h, w in sizes), dtype=torch.float32, device=frames.device)
    canvas = torch.empty((n, 640, 640, 3), dtype=torch.uint8, device=frames.device)
    rc = lib().frt_detector_forward(handle.h, _p(frames), n, H, W, _p(heads), _p(canvas),
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, handle.h)
    out, off = [], 0
    for h, w in sizes:
        out.append(heads[off:off + n * h * w * 32].view(n, h, w, 32))
        off += n * h * w * 32
    return out, canvas


def set_detector_row_reduction(handle, on):
    _lib.check(lib().frt_set_detector_row_reduction(handle.h, int(on)), handle.h)


def conv2d_s2band(x, w, B, H, W, post, res, out=None):
    """The stage-1 stride-2 band conv: x, res NHWC [B,H,W,64] cuda f32, w [64][3][3][64].
    out: the caller's buffer instead of a fresh NaN-filled one (a test of a refusal)."""
    y = torch.full((B, H // 2, W // 2, 64), float("nan"), device=x.device) if out is None else out
    rc = lib().frt_conv2d_s2band(_p(x), _p(w), _p(y), B, H, W, _p(post[0]), _p(post[1]), _p(res),
                                 torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return y


def conv2d_small(x, w, B, H, W, cin, cout, stride=1, x2=None, cin2=0, pre=None, post=None, prelu=None, res=None,
                 epi=0, blk=0, y2=None, out=None):
    """conv_small.hip's serving kernel: x NHWC cuda f32, w [cout][9*cin + cin2] cuda f32.
    blk: the CONVS_BLK_* tensors are handed to the kernel channel-blocked (x, x2 and res are blocked
    here, y and y2 unblocked here: NHWC in and out).  y2: None, or (scale, shift) of the second
    output, either of which may be None (a refusal); the call then returns (y, y2).
    out: the caller's y buffer instead of a fresh NaN-filled one (returned as the kernel left it)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.full((B, Ho, Wo, cout), float("nan"), device=w.device) if out is None else out
    assert y.shape == (B, Ho, Wo, cout) and y.dtype == torch.float32 and y.is_contiguous()
    ps, ph = (pre if pre is not None else (None, None))
    qs, qh = post
    x, x2, res = _as(x, blk & CONVS_BLK_X), _as(x2, blk & CONVS_BLK_X2), _as(res, blk & CONVS_BLK_RES)
    y2b, (s2, t2) = None, (None, None)
    if y2 is not None:
        y2b, (s2, t2) = torch.full_like(y, float("nan")), y2
    rc = lib().frt_conv2d_small_ex(_p(x), _p(x2), _p(w), _p(y), B, H, W, cin, cin2, cout, stride, _p(ps), _p(ph),
                                   _p(qs), _p(qh), _p(prelu), _p(res), epi, blk, _p(y2b), _p(s2), _p(t2),
                                   torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    if out is None:
        y = _unblock(y, blk & CONVS_BLK_Y)
    return y if y2 is None else (y, _unblock(y2b, blk & CONVS_BLK_Y))
