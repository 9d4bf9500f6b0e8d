"""head_reduce_kernel, stem_kernel<16> and the band kernel on non-square maps, each alone against
float64 from the same f32 inputs.

head_reduce_kernel had no entry point: the network runs it at nsplit 32 and 98 with split_stride =
n * 512 only.  Its plain (no norm) output is held to the rounding bound of what it computes, a
recursive f32 sum of nsplit partials and the bias followed by one affine:
    |d| <= (nsplit + 3) * 2^-24 * (sum_s |partial_s| + |bias|) * |bn_scale| + 2^-24 * |ref|
(at most nsplit inexact additions whatever the grouping -- the first of a group adds to 0 -- and
up to two roundings of the affine's product and sum if it is not one fma; the last term is the final
rounding).  The normalised outputs take the project's bar, 1e-5 * max|ref| + 1e-6.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import _frt
from tests.test_gpu_kernels import _close, _nhwc, _rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
N = 3  # embedding rows


def _head_inputs(nsplit, stride, seed, scale_row=None):
    part = _rand(nsplit * stride, seed=seed)
    if scale_row is not None:
        row, s = scale_row
        part.view(nsplit, stride)[:, row * 512:(row + 1) * 512] *= s
    bias = _rand(512, seed=seed + 1, lo=-0.5, hi=0.5)
    sc, sh = _rand(512, seed=seed + 2, lo=0.5, hi=1.5), _rand(512, seed=seed + 3, lo=-0.2, hi=0.2)
    return part, bias, sc, sh


def _head_ref(part, nsplit, stride, bias, sc, sh, normalize, model_l2):
    """float64 tail of the network from the same f32 partials -> (ref [N][512], rounding bound of the
    plain output [N][512])."""
    p = part.double().view(nsplit, stride)[:, :N * 512].reshape(nsplit, N, 512)
    v = (p.sum(0) + bias.double()) * sc.double() + sh.double()
    bound = (nsplit + 3) * U * (p.abs().sum(0) + bias.double().abs()) * sc.double().abs() + U * v.abs()
    if model_l2:
        v = v / v.norm(dim=1, keepdim=True)
    if normalize:
        v = v / (v.norm(dim=1, keepdim=True) + 1e-8)
    return v, bound


@pytest.mark.parametrize("pad", [0, 512])
@pytest.mark.parametrize("nsplit", [1, 2, 3, 4, 7, 32, 33, 49, 98, 196])
def test_head_reduce(nsplit, pad):
    """Split counts that leave groups empty (1, 2, 3), give each one split (4), ragged groups with
    and without an 8-wide tail (7, 33, 49, 98), whole unrolled rounds (32, 196); split_stride = n * 512
    and padded by one row (a stride taken for the row count reads the wrong slab); all four flag
    pairs; each launched twice (bitwise equal: the group sums are added in a fixed order)."""
    stride = N * 512 + pad
    part, bias, sc, sh = _head_inputs(nsplit, stride, seed=2000 + nsplit)
    dv = [t.to(DEV) for t in (part, bias, sc, sh)]
    for normalize, model_l2 in ((0, 0), (0, 1), (1, 0), (1, 1)):
        ref, bound = _head_ref(part, nsplit, stride, bias, sc, sh, normalize, model_l2)
        got = _frt.head_reduce(dv[0], nsplit, stride, dv[1], dv[2], dv[3], N, normalize, model_l2)
        again = _frt.head_reduce(dv[0], nsplit, stride, dv[1], dv[2], dv[3], N, normalize, model_l2)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all()
        assert torch.equal(got, again), "head_reduce is not run-to-run deterministic"
        d = (got.cpu().double() - ref).abs()
        if not normalize and not model_l2:
            worst = (d / bound).max().item()
            assert worst <= 1.0, f"|diff| is {worst:.2f} x the rounding bound"
        else:
            _close(got.cpu(), ref)


@pytest.mark.parametrize("nsplit", [1, 7])
def test_head_reduce_tiny_row_shows_the_epsilon(nsplit):
    """A row whose partials are scaled by 1e-9 (no bias, no BN shift): ||e|| is about 1e-8, so
    e / (||e|| + 1e-8) is about half of e / ||e||.  Flags (normalize 1, model_l2 0) within 1e-4 of the
    row's largest float64 element (elements that cancel to near zero have no relative accuracy of
    their own; the f32 sum of nsplit terms and the norm of 512 squares err by ~1e-6 relative)."""
    stride = N * 512
    part, bias, sc, sh = _head_inputs(nsplit, stride, seed=2100 + nsplit, scale_row=(1, 1e-9))
    bias.zero_()
    sh.zero_()
    ref, _ = _head_ref(part, nsplit, stride, bias, sc, sh, 1, 0)
    e = (part.double().view(nsplit, N, 512).sum(0) * sc.double())[1]
    assert 3e-9 < e.norm().item() < 1e-7  # the planted row is where the + 1e-8 matters
    got = _frt.head_reduce(part.to(DEV), nsplit, stride, bias.to(DEV), sc.to(DEV), sh.to(DEV), N, 1, 0)
    torch.cuda.synchronize()
    d = (got.cpu().double() - ref).abs()
    assert torch.isfinite(got).all()
    for row in range(N):
        assert d[row].max().item() <= 1e-4 * ref[row].abs().max().item(), row


def test_head_reduce_refusals():
    stride = N * 512
    part, bias, sc, sh = (t.to(DEV) for t in _head_inputs(4, stride, seed=2200))
    for kw in (dict(nsplit=0), dict(stride=stride - 1), dict(stride=512), dict(partial=None), dict(bias=None),
               dict(sc=None), dict(sh=None), dict(n=0)):
        a = dict(partial=part, nsplit=4, stride=stride, bias=bias, sc=sc, sh=sh, n=N)
        a.update(kw)
        out = torch.full((N, 512), float("nan"), device=DEV)
        with pytest.raises(ValueError):
            _frt.head_reduce(a["partial"], a["nsplit"], a["stride"], a["bias"], a["sc"], a["sh"], a["n"], 1, 1, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), kw
    # no output pointer (the wrapper always has one: the C call itself)
    assert _frt.lib().frt_head_reduce(part.data_ptr(), 4, stride, bias.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, N,
                                      1, 1, None) != 0


def test_stem_batch_instances():
    """B = 8 runs stem_kernel<4> (4 output rows per workgroup), B = 9 stem_kernel<16>: both against
    float64 on the same LUT-normalised input, and images 0..7 of the two launches bitwise equal (each
    output is the same fmaf chain whatever the rows per workgroup)."""
    from oracle.reference_path import preprocess, preprocess_lut
    from facerecognitionpipeline_amd.weights import synthetic_crops
    imgs = synthetic_crops(9, seed=321)
    w = _rand(64, 3, 3, 3, seed=2300) / 27 ** 0.5
    sc, sh = _rand(64, seed=2301, lo=0.5, hi=1.5), _rand(64, seed=2302, lo=-0.2, hi=0.2)
    al = _rand(64, seed=2303, lo=0.1, hi=0.4)

    def c(v):
        return v.double().view(1, -1, 1, 1)
    x = torch.cat([preprocess(i) for i in imgs]).double()
    ref = F.conv2d(x, w.double(), padding=1) * c(sc) + c(sh)
    ref = _nhwc(torch.where(ref > 0, ref, ref * c(al)))
    w27 = torch.empty(3, 3, 3, 64)
    for ch in range(3):  # tensor channel ch (BGR) is RGB channel 2 - ch
        w27[:, :, 2 - ch, :] = w[:, ch].permute(1, 2, 0)
    dv = [t.to(DEV) for t in (torch.from_numpy(preprocess_lut()), w27.reshape(27, 64).contiguous(), sc, sh, al)]
    img = torch.from_numpy(imgs).to(DEV)
    got9 = _frt.stem(img, *dv)
    got8 = _frt.stem(img[:8].contiguous(), *dv)
    torch.cuda.synchronize()
    assert torch.isfinite(got9).all() and torch.isfinite(got8).all()
    assert torch.equal(got9[:8], got8), "stem_kernel<16> and <4> differ on the same images"
    _close(got9.cpu(), ref)
    _close(got8.cpu(), ref[:8])


def _band_inputs(B, H, W, seed):
    x = _rand(B, 64, H, W, seed=seed)
    w = _rand(64, 64, 3, 3, seed=seed + 1) / (64 * 9) ** 0.5
    post = (_rand(64, seed=seed + 4, lo=0.5, hi=1.5), _rand(64, seed=seed + 5, lo=-0.2, hi=0.2))
    return x, w, post


@pytest.mark.parametrize("B,H,W", [(2, 6, 16), (1, 2, 112), (3, 10, 30), (1, 112, 16)])
def test_band_kernel_non_square(B, H, W):
    """s2c64_kernel where H != W: the minimum width (Wo = 8: half a 16-pixel block per output row),
    one band of the full width, Wo = 15 with an odd band count (Ho = 5), tall and narrow."""
    x, w, post = _band_inputs(B, H, W, 2400 + H + W)
    ref = F.conv2d(x.double(), w.double(), stride=2, padding=1) * post[0].double().view(1, -1, 1, 1)
    ref = ref + post[1].double().view(1, -1, 1, 1) + x.double()[:, :, ::2, ::2]
    xd = _nhwc(x).to(DEV)
    got = _frt.conv2d_s2band(xd, w.permute(0, 2, 3, 1).contiguous().to(DEV), B, H, W,
                             (post[0].to(DEV), post[1].to(DEV)), xd)
    torch.cuda.synchronize()
    assert got.shape == (B, H // 2, W // 2, 64) and torch.isfinite(got).all()
    _close(got.cpu(), _nhwc(ref))


@pytest.mark.parametrize("H,W", [(6, 14), (6, 114), (7, 16)])
def test_band_kernel_refusals(H, W):
    """Wo = 7 (below the 8 a staged row needs), Wo = 57 (past the 113 staged columns), odd H."""
    x, w, post = _band_inputs(1, H, W, 2500)
    xd = _nhwc(x).to(DEV)
    out = torch.full((1, H // 2, W // 2, 64), float("nan"), device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        _frt.conv2d_s2band(xd, w.permute(0, 2, 3, 1).contiguous().to(DEV), 1, H, W,
                           (post[0].to(DEV), post[1].to(DEV)), xd, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
