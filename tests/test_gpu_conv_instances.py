"""The implicit-GEMM conv paths (conv_mfma_impl.h, conv_mfma.hip) that only whole-network tests reached.

A. the detector's instance set (conv_det.hip: tiles 6, 7, 8; epi=1 without pre-BN and epi=5),
B. the MFMA kernel's fused 1x1 shortcut (ConvParams::x2 / Cin2 / steps1, cin2= below),
C. conv_split_fixup_kernel (the serving path of every stride-2 conv2), alone on planted slabs and
   behind the EPI_RAW split-K launch it finishes in production.
(D, non-square maps on the embedding instances, and E, the tile lists, are in test_gpu_kernels.py.)

Reference: the same operation in float64 on the CPU, from the exact f32 inputs (fused shortcut, post
affine, residual and PReLU included), so the reference's own rounding (~1e-16 relative) takes none of
the bar.  Bar: the project's, |d| <= 1e-5 * max|ref| + 1e-6 (test_gpu_kernels._close): the kernels
compute exact f32 products with f32 accumulation, only the summation order differs.
Shapes are tiny on purpose: ragged against every tile edge, odd and non-square maps.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facerecognitionpipeline_amd._lib import FrHipError
from tests import _frt

pytestmark = pytest.mark.gpu
DEV = "cuda"
REFUSED = (ValueError, FrHipError)
ALL_TILES = list(range(11))
# every tile runs the stream-K schedule (test_gpu_kernels.test_stream_k_schedule_matches_and_is_deterministic)
STREAM_K_TILES = list(range(11))


def _rand(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _c(v):
    return v.double().view(1, -1, 1, 1)


def _close(got, ref, rel=1e-5):
    """got f32 (NHWC, any device) against the float64 reference (NHWC) at the project's bar."""
    ref = ref.double()
    tol = rel * ref.abs().max().item() + 1e-6
    g = got.detach().cpu().double()
    assert g.shape == ref.shape
    assert not torch.isnan(g).any(), "output holds NaN: elements the kernel never wrote"
    d = (g - ref).abs().max().item()
    assert d <= tol, f"max |diff| {d:.3e} > tol {tol:.3e}"


def _untouched(y):
    torch.cuda.synchronize()
    assert torch.isnan(y).all().item(), "a refused launch wrote to its output"


# ---------------------------------------------------------------------------------------------
# A. detector instances: launch_conv -> launch_conv_det -> launch_tile<..., SET = 1>
# ---------------------------------------------------------------------------------------------
DET_SHAPES = {
    # M = 280: ragged against 128 and 256; N = 96: ragged against 64 and 128; 18 K-steps: the
    # stream-K schedule cuts every tile across blocks
    "3x3s1": (2, 10, 14, 64, 96, 3, 1, 1),
    # odd height, M = 3 * 6 * 7 = 126 < one tile
    "3x3s2": (3, 11, 14, 32, 224, 3, 2, 1),
    "1x1": (2, 6, 9, 96, 64, 1, 1, 0),
}


@functools.lru_cache(maxsize=None)
def _det_case(name, epi):
    """Inputs (device, NHWC) and the float64 reference of one detector conv, built once per (shape, epi)."""
    B, H, W, cin, cout, k, stride, pad = DET_SHAPES[name]
    seed = 1000 + 10 * sorted(DET_SHAPES).index(name) + epi
    x = _rand(B, cin, H, W, seed=seed)  # centred on zero: both PReLU branches occur
    w = _rand(cout, cin, k, k, seed=seed + 1) / (cin * k * k) ** 0.5
    post_s, post_b = _rand(cout, seed=seed + 2, lo=0.5, hi=1.5), _rand(cout, seed=seed + 3, lo=-0.2, hi=0.2)
    al = _rand(cout, seed=seed + 4, lo=0.1, hi=0.4)
    al[::2] = 0.0  # the detector's ReLU is a PReLU of slope exactly zero
    v = F.conv2d(x.double(), w.double(), stride=stride, padding=pad) * _c(post_s) + _c(post_b)
    res = None
    if epi == 5:
        r = _rand(*v.shape, seed=seed + 5)  # of the conv's own magnitude: dropping it misses the bar ~1e4 times over
        v = v + r.double()
        res = _nhwc(r).to(DEV)
    ref = torch.where(v > 0, v, v * _c(al))
    # both branches, on the ReLU channels and on the sloped ones
    for grp in (slice(0, None, 2), slice(1, None, 2)):
        assert (v[:, grp] > 0).any() and (v[:, grp] < 0).any()
    dev = dict(x=_nhwc(x).to(DEV), w=w.permute(0, 2, 3, 1).contiguous().to(DEV), post=(post_s.to(DEV), post_b.to(DEV)),
               prelu=al.to(DEV), res=res)
    return dev, _nhwc(ref)


def _det_launch(name, epi, tile, stream_k=0, out=None, override=None):
    B, H, W, cin, cout, k, stride, pad = DET_SHAPES[name]
    d, _ = _det_case(name, epi)
    kw = dict(pre=None, post=d["post"], prelu=d["prelu"], res=d["res"], epi=epi, tile=tile, stream_k=stream_k, out=out)
    kw.update(override or {})
    return _frt.conv2d(d["x"], d["w"], B, H, W, cin, cout, k, k, stride, pad, **kw)


@pytest.mark.parametrize("name", sorted(DET_SHAPES))
@pytest.mark.parametrize("epi", [1, 5])
@pytest.mark.parametrize("tile", [6, 7, 8])
def test_detector_instances(tile, epi, name):
    """epi=1 without pre-BN (conv + BN + ReLU) and epi=5 (conv2 + BN + residual + ReLU) on each tile of
    conv_det.hip, in grid mode and on the stream-K schedule (twice: bitwise the same)."""
    _, ref = _det_case(name, epi)
    _close(_det_launch(name, epi, tile), ref)
    a = _det_launch(name, epi, tile, stream_k=1)
    b = _det_launch(name, epi, tile, stream_k=1)
    _close(a, ref)
    assert torch.equal(a, b), "stream-K result depends on arrival order"


@pytest.mark.parametrize("epi", [1, 5])
def test_detector_epilogues_refused_off_their_tiles(epi):
    """conv_det.hip has three tiles: run_conv's `!h->detector` guards keep TILE_64x128 and the fused-
    shortcut tile knob away from the detector because any other tile is refused, not run elsewhere."""
    B, H, W, cin, cout, k, stride, pad = DET_SHAPES["1x1"]
    for tile in (0, 1, 2, 3, 4, 5, 9, 10):
        for sk in (0, 1):
            y = torch.full((1, B, H, W, cout), float("nan"), device=DEV)
            with pytest.raises(REFUSED):
                _det_launch("1x1", epi, tile, stream_k=sk, out=y)
            _untouched(y)


def test_detector_epilogues_need_their_pointers():
    """frt_conv2d turns a missing pointer into FR_ERR_INVALID_ARGUMENT before any launch."""
    B, H, W, cin, cout, k, stride, pad = DET_SHAPES["1x1"]
    d, _ = _det_case("1x1", 5)
    pre = (torch.ones(cin, device=DEV), torch.zeros(cin, device=DEV))
    bad = [dict(epi=5, res=None), dict(epi=5, prelu=None), dict(epi=5, post=None), dict(epi=5, pre=pre),
           dict(epi=1, prelu=None), dict(epi=1, post=None), dict(epi=1, pre=(pre[0], None)),
           dict(epi=2, res=None), dict(epi=3, res=None), dict(epi=0, post=None)]
    for kw in bad:
        y = torch.full((1, B, H, W, cout), float("nan"), device=DEV)
        with pytest.raises(ValueError):
            _det_launch("1x1", 5, 6, out=y, override=kw)
        _untouched(y)


# ---------------------------------------------------------------------------------------------
# B. the fused 1x1 shortcut of the MFMA kernel: K-steps [steps1, steps_total) read x2
# ---------------------------------------------------------------------------------------------
FUSED_SHAPES = {
    # B, H, W, cin, cin2, cout, stride
    "s2": (2, 14, 10, 64, 32, 96, 2),   # 18 + 1 = 19 K-steps, M = 2 * 7 * 5 = 70
    "s1": (1, 9, 9, 32, 64, 160, 1),    # 9 + 2 K-steps: two shortcut steps, M = 81
    "sub": (2, 15, 10, 64, 32, 64, 2),  # epi 3: res = x at (2 oy, 2 ox), odd res height 15
}
FUSED_CASES = [("s2", 0), ("s2", 2), ("s1", 0), ("s1", 2), ("sub", 3)]


@functools.lru_cache(maxsize=None)
def _fused_case(name, epi):
    """Inputs (device) and the float64 reference conv3x3(x) + conv1x1(x2, stride) -> epilogue; epi 4: raw."""
    B, H, W, cin, cin2, cout, stride = FUSED_SHAPES[name]
    seed = 2000 + 10 * sorted(FUSED_SHAPES).index(name)  # the same tensors for every epilogue of a shape
    x = _rand(B, cin, H, W, seed=seed)
    x2 = _rand(B, cin2, H, W, seed=seed + 50)  # its own seed: reading x for x2 cannot pass
    w = _rand(cout, cin, 3, 3, seed=seed + 1) / (cin * 9) ** 0.5
    # the shortcut's columns weigh as much as the whole 3x3 conv: dropping or misplacing its K-steps
    # changes outputs by ~0.3, four orders over the bar
    w2 = _rand(cout, cin2, seed=seed + 51) / cin2 ** 0.5
    post_s, post_b = _rand(cout, seed=seed + 2, lo=0.5, hi=1.5), _rand(cout, seed=seed + 3, lo=-0.2, hi=0.2)
    main = F.conv2d(x.double(), w.double(), stride=stride, padding=1)
    sc = F.conv2d(x2.double(), w2.double().view(cout, cin2, 1, 1), stride=stride)
    assert sc.abs().max() > 0.1 * main.abs().max()
    v = main + sc
    res, res_hw = None, (0, 0)
    if epi != 4:
        v = v * _c(post_s) + _c(post_b)
    if epi == 2:
        r = _rand(*v.shape, seed=seed + 5)
        v = v + r.double()
        res = _nhwc(r).to(DEV)
    if epi == 3:
        assert cin == cout and stride == 2
        v = v + x.double()[:, :, ::2, ::2]
        res, res_hw = _nhwc(x).to(DEV), (H, W)
    wk = torch.cat([w.permute(0, 2, 3, 1).reshape(cout, 9 * cin), w2], 1).contiguous()
    dev = dict(x=_nhwc(x).to(DEV), x2=_nhwc(x2).to(DEV), w=wk.to(DEV), post=(post_s.to(DEV), post_b.to(DEV)),
               res=res, res_hw=res_hw)
    return dev, _nhwc(v)


def _fused_launch(name, epi, tile, **kw):
    B, H, W, cin, cin2, cout, stride = FUSED_SHAPES[name]
    d, _ = _fused_case(name, epi)
    args = dict(post=d["post"] if epi != 4 else None, res=d["res"], res_hw=d["res_hw"], epi=epi, tile=tile)
    args.update(kw)
    return _frt.conv2d_fused(d["x"], d["x2"], d["w"], B, H, W, cin, cin2, cout, 3, 3, stride, 1, **args)


@pytest.mark.parametrize("name,epi", FUSED_CASES)
@pytest.mark.parametrize("tile", ALL_TILES)
def test_fused_shortcut_every_tile(tile, name, epi):
    """cin2= 32 / 64 on every tile in grid mode, and on the stream-K schedule (twice, bitwise equal)."""
    _, ref = _fused_case(name, epi)
    _close(_fused_launch(name, epi, tile), ref)
    if tile in STREAM_K_TILES:
        a = _fused_launch(name, epi, tile, stream_k=1)
        b = _fused_launch(name, epi, tile, stream_k=1)
        _close(a, ref)
        assert torch.equal(a, b), "stream-K result depends on arrival order"


@pytest.mark.parametrize("tile", [3, 8])
@pytest.mark.parametrize("nsplit", [2, 3, 5, 6])
def test_fused_shortcut_split_k(nsplit, tile):
    """epi=4 slabs of the 19-step conv (18 main K-steps + 1 shortcut step), summed, against the raw
    reference.  ceil(19 / nsplit) = 10, 7, 4 steps per split for nsplit 2, 3, 5: the last split is
    steps [10, 19), [14, 19), [16, 19), the shortcut step with 8, 4 and 2 main steps before it.
    nsplit 6 also runs 4 steps per split, so its sixth split starts at step 20 and is empty (run_conv
    recomputes S and never launches one): the kernel's rule for it is a slab of zeros, pinned here."""
    per = -(-19 // nsplit)
    empty = [s for s in range(nsplit) if s * per >= 19]
    assert empty == ([5] if nsplit == 6 else [])
    _, ref = _fused_case("s2", 4)
    slabs = _fused_launch("s2", 4, tile, nsplit=nsplit)
    torch.cuda.synchronize()
    assert slabs.shape[0] == nsplit
    for s in empty:
        assert (slabs[s] == 0).all().item()
    _close(slabs.double().sum(0).float(), ref)


def test_fused_shortcut_refusals():
    """launch_conv's rules for cin2 > 0: whole 32-channel K-steps, no pre-BN, not on the detector's epilogues."""
    B, H, W, cin, cin2, cout, stride = FUSED_SHAPES["s2"]
    d, _ = _fused_case("s2", 2)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pre = (torch.ones(cin, device=DEV), torch.zeros(cin, device=DEV))
    prelu = torch.full((cout,), 0.25, device=DEV)
    r = torch.zeros(B, Ho, Wo, cout, device=DEV)

    def refused(x2, w, c2, **kw):
        y = torch.full((1, B, Ho, Wo, cout), float("nan"), device=DEV)
        with pytest.raises(REFUSED):
            _frt.conv2d_fused(d["x"], x2, w, B, H, W, cin, c2, cout, 3, 3, stride, 1, post=d["post"], out=y, **kw)
        _untouched(y)

    x2_16 = d["x2"][..., :16].contiguous()
    w_16 = d["w"][:, :9 * cin + 16].contiguous()
    for tile in (1, 6):
        refused(x2_16, w_16, 16, epi=0, tile=tile)                      # cin2=16: half a K-step
        refused(d["x2"], d["w"], cin2, epi=0, pre=pre, tile=tile)       # pre-BN with cin2=32
        refused(d["x2"], d["w"], cin2, epi=1, prelu=prelu, tile=tile)   # detector conv + ReLU
        refused(d["x2"], d["w"], cin2, epi=1, prelu=prelu, pre=pre, tile=tile)
        refused(d["x2"], d["w"], cin2, epi=5, prelu=prelu, res=r, tile=tile)
    refused(None, d["w"], cin2, epi=0, tile=1)                          # cin2=32 without x2


# ---------------------------------------------------------------------------------------------
# C. conv_split_fixup_kernel
# ---------------------------------------------------------------------------------------------
FIX = dict(B=1, Ho=7, Wo=9, cout=48)  # M * Cout = 3024: 11 whole blocks of 256 threads + 208
FIX_RES_HW = (13, 18)                 # odd and non-square; (2 * 6, 2 * 8) is its last pixel


@functools.lru_cache(maxsize=None)
def _planted(S):
    """S planted slabs `stride` apart in a NaN-filled buffer with one more (NaN) slab behind them."""
    n = FIX["B"] * FIX["Ho"] * FIX["Wo"] * FIX["cout"]
    stride = n + 40
    slabs = _rand(S, n, seed=3000 + S)
    part = torch.full(((S + 1) * stride,), float("nan"))
    for s in range(S):
        part[s * stride:s * stride + n] = slabs[s]
    return slabs, part.to(DEV), stride


@pytest.mark.parametrize("epi", [0, 2, 3])
@pytest.mark.parametrize("S", [1, 2, 5, 31, 32])
def test_split_fixup_planted_slabs(S, epi):
    """split_fixup on planted slabs against float64.  Bar: a sequential f32 sum of S <= 32 terms rounds
    each add to half an ulp of a partial sum <= max|ref|, so |d| <= 32 * 2^-24 * max|ref| = 1.9e-6 *
    max|ref| before the affine: inside the project's 1e-5 * max|ref| + 1e-6."""
    B, Ho, Wo, cout = FIX["B"], FIX["Ho"], FIX["Wo"], FIX["cout"]
    slabs, part, stride = _planted(S)
    post_s, post_b = _rand(cout, seed=3100, lo=0.5, hi=1.5), _rand(cout, seed=3101, lo=-0.2, hi=0.2)
    ref = slabs.double().sum(0).view(B, Ho, Wo, cout) * post_s.double() + post_b.double()
    res, res_hw = None, (0, 0)
    if epi == 2:
        r = _rand(B, Ho, Wo, cout, seed=3102)
        ref = ref + r.double()
        res = r.to(DEV)
    if epi == 3:
        res_hw = FIX_RES_HW
        r = _rand(B, res_hw[0], res_hw[1], cout, seed=3103)
        ref = ref + r.double()[:, ::2, ::2][:, :Ho, :Wo]
        res = r.to(DEV)
    got = _frt.conv_split_fixup(part, S, stride, B, Ho, Wo, cout, (post_s.to(DEV), post_b.to(DEV)), res=res,
                                res_hw=res_hw, epi=epi)
    torch.cuda.synchronize()
    _close(got, ref)


@pytest.mark.parametrize("S", [1, 2, 5, 31, 32])
def test_split_fixup_sums_in_split_order(S):
    """The header's promise: the slabs are summed in split order.  With scale 1, shift 0 and epi=0 the
    output is bitwise numpy's sequential f32 sum (v * 1 + 0 is exact, fused or not)."""
    B, Ho, Wo, cout = FIX["B"], FIX["Ho"], FIX["Wo"], FIX["cout"]
    slabs, part, stride = _planted(S)
    acc = np.zeros(slabs.shape[1], dtype=np.float32)
    for s in range(S):
        acc = acc + slabs[s].numpy()
    assert acc.dtype == np.float32
    one, zero = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    got = _frt.conv_split_fixup(part, S, stride, B, Ho, Wo, cout, (one, zero), epi=0)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.int32), acc.view(np.int32))


def test_split_fixup_refusals():
    """S outside [1, 32] (the kernel keeps 32 slab values in registers) and epilogues it has no instance of."""
    B, Ho, Wo, cout = FIX["B"], FIX["Ho"], FIX["Wo"], FIX["cout"]
    _, part, stride = _planted(32)
    one, zero = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    r = torch.zeros(B, Ho, Wo, cout, device=DEV)
    for kw in (dict(S=0), dict(S=33), dict(S=-1), dict(S=2, epi=1), dict(S=2, epi=4), dict(S=2, epi=5, res=r),
               dict(S=2, epi=2), dict(S=2, epi=3, res=r, res_hw=(12, 18)), dict(S=2, epi=3, res=r, res_hw=(13, 16))):
        y = torch.full((B, Ho, Wo, cout), float("nan"), device=DEV)
        args = dict(epi=0)
        args.update(kw)
        S = args.pop("S")
        with pytest.raises(ValueError):
            _frt.conv_split_fixup(part, S, stride, B, Ho, Wo, cout, (one, zero), out=y, **args)
        _untouched(y)


@pytest.mark.parametrize("name,epi", [("s2", 0), ("s2", 2), ("sub", 3)])
def test_split_k_then_fixup_as_serving_runs_it(name, epi):
    """run_conv's serving path of a stride-2 conv2 (+ fused shortcut): an EPI_RAW launch of S splits
    on TILE_64x128, then split_fixup with the layer's epilogue.  S as run_conv computes it for the
    19 K-steps: min(32, 19 // 4) = 4 -> 5 steps per split -> S = ceil(19 / 5) = 4."""
    B, H, W, cin, cin2, cout, stride = FUSED_SHAPES[name]
    d, ref = _fused_case(name, epi)
    steps = 9 * cin // 32 + cin2 // 32
    S = min(32, steps // 4)
    per = -(-steps // S)
    S = -(-steps // per)
    assert (steps, S) == (19, 4)
    slabs = _fused_launch(name, 4, 3, nsplit=S, post=None, res=None, res_hw=(0, 0))
    Ho, Wo = slabs.shape[2], slabs.shape[3]
    got = _frt.conv_split_fixup(slabs, S, B * Ho * Wo * cout, B, Ho, Wo, cout, d["post"], res=d["res"],
                                res_hw=d["res_hw"], epi=epi)
    torch.cuda.synchronize()
    _close(got, ref)
