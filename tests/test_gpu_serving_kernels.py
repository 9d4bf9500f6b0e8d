"""conv_small.hip's serving kernel alone, on what only whole-network tests on square maps reached:
channel-blocked activations (ConvParams::blk), the second output y2 = BN_next(y), conv1 without
pre-BN (the instance that reads y2), the widths of the fused shortcut, the fill edges of the
register ring, and launch_convs' refusals.

The reference is float64 from the same f32 inputs; the bar is the project's,
|d| <= 1e-5 * max|ref| + 1e-6 (tests/test_gpu_kernels.py: exact f32 products, f32 accumulation, only
the summation order differs).  A layout changes addresses, never arithmetic, so every blocked launch
must also be bitwise the NHWC launch of the same tensors.  Maps are non-square (every blocked
stride is H * W * 16: an H / W slip or Ho * Wo for res_H * res_W cannot show on a square one) and
small: at most 400 pixels and 256 channels.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _frt
from tests._frt import CONVS_BLK_RES, CONVS_BLK_X, CONVS_BLK_X2, CONVS_BLK_Y
from tests.test_gpu_kernels import _close, _nhwc, _rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
REFUSED = (ValueError, RuntimeError)  # FR_ERR_INVALID_ARGUMENT, FR_ERR_HIP

# each bit alone, then what plan_layouts produces: conv1 X|Y, conv2 X|X2|RES|Y, X2|RES (a block whose
# conv1 is not on this kernel), X alone and Y alone (the ends of a run of blocked layers)
LAYOUTS = [CONVS_BLK_X, CONVS_BLK_X2, CONVS_BLK_RES, CONVS_BLK_Y, CONVS_BLK_X | CONVS_BLK_Y,
           CONVS_BLK_X | CONVS_BLK_X2 | CONVS_BLK_RES | CONVS_BLK_Y, CONVS_BLK_X2 | CONVS_BLK_RES]


def _c(v):
    return v.double().view(1, -1, 1, 1)


@functools.lru_cache(maxsize=8)
def _case(B, H, W, cin, cout, stride, cin2, epi, pre, seed):
    """The f32 tensors of one launch (CPU; activations NHWC, w [cout][9 cin + cin2]) and its float64
    reference (NHWC), computed once for the launches that share them and never changed.
    The residual of epi 3 is a tensor of its own, [B][H][W][cout] read at (stride oy, stride ox)."""
    x = _rand(B, cin, H, W, seed=seed)
    w = _rand(cout, cin, 3, 3, seed=seed + 1) / (cin * 9) ** 0.5
    pre_s, pre_b = _rand(cin, seed=seed + 2, lo=0.5, hi=1.5), _rand(cin, seed=seed + 3, lo=-0.2, hi=0.2)
    post_s, post_b = _rand(cout, seed=seed + 4, lo=0.5, hi=1.5), _rand(cout, seed=seed + 5, lo=-0.2, hi=0.2)
    al = _rand(cout, seed=seed + 6, lo=0.1, hi=0.4)
    xin = x.double() * _c(pre_s) + _c(pre_b) if pre else x.double()
    acc = F.conv2d(xin, w.double(), stride=stride, padding=1)
    wk = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    t = {"x": _nhwc(x), "pre": (pre_s, pre_b) if pre else None, "post": (post_s, post_b),
         "prelu": al if epi == 1 else None, "x2": None, "res": None}
    if cin2:
        x2 = _rand(B, cin2, H, W, seed=seed + 8)
        w2 = _rand(cout, cin2, seed=seed + 9) / cin2 ** 0.5
        acc = acc + F.conv2d(x2.double(), w2.double().view(cout, cin2, 1, 1), stride=stride)
        wk = torch.cat([wk, w2], 1)
        t["x2"] = _nhwc(x2)
    t["w"] = wk.contiguous()
    ref = acc * _c(post_s) + _c(post_b)
    if epi == 1:
        ref = torch.where(ref > 0, ref, ref * _c(al))
    if epi == 2:
        r = _rand(B, cout, ref.shape[2], ref.shape[3], seed=seed + 7)
        ref = ref + r.double()
        t["res"] = _nhwc(r)
    if epi == 3:
        r = _rand(B, cout, H, W, seed=seed + 7)
        ref = ref + r.double()[:, :, ::stride, ::stride]
        t["res"] = _nhwc(r)
    return t, _nhwc(ref)


def _dev(t):
    def d(v):
        return v if v is None else tuple(e.to(DEV) for e in v) if isinstance(v, tuple) else v.to(DEV)
    return {k: d(v) for k, v in t.items()}


def _launch(d, shape, blk=0, y2=None, out=None):
    """One launch on the device tensors of _dev(_case(*shape)...): y (NHWC, on the CPU), or (y, y2)."""
    B, H, W, cin, cout, stride, cin2, epi = shape
    got = _frt.conv2d_small(d["x"], d["w"], B, H, W, cin, cout, stride=stride, x2=d["x2"], cin2=cin2, pre=d["pre"],
                            post=d["post"], prelu=d["prelu"], res=d["res"], epi=epi, blk=blk, y2=y2, out=out)
    torch.cuda.synchronize()
    return tuple(g.cpu() for g in got) if isinstance(got, tuple) else got.cpu()


def _present(shape):
    """The CONVS_BLK_* bits whose tensor this launch has."""
    cin2, epi = shape[6], shape[7]
    return CONVS_BLK_X | CONVS_BLK_Y | (CONVS_BLK_X2 if cin2 else 0) | (CONVS_BLK_RES if epi in (2, 3) else 0)


def _layout_sweep(shape, pre, seed, layouts=LAYOUTS):
    t, ref = _case(*shape, pre, seed)
    d = _dev(t)
    base = _launch(d, shape)
    assert base.shape == ref.shape
    _close(base, ref)
    done = {0}
    for blk in layouts:
        eff = blk & _present(shape)  # a bit of a tensor the launch does not have changes nothing
        if eff in done:
            continue
        done.add(eff)
        got = _launch(d, shape, blk=eff)
        assert torch.isfinite(got).all(), f"blk {eff}: an output element was not written"
        _close(got, ref)
        assert torch.equal(got, base), f"blk {eff}: not bitwise the NHWC launch"
    return len(done) - 1


# (epi, pre-BN, cin2): conv2 + fused conv shortcut, conv1 with pre-BN, conv1 on a y2 input (no pre-BN),
# conv2 + identity residual, conv2 + MaxPool2d(1, s) shortcut
EPIS = [(0, False, 32), (1, True, 0), (1, False, 0), (2, False, 0), (3, False, 0)]


@pytest.mark.parametrize("cout", [48, 128])  # plain block order; NCB % 8 == 0: the XCD order
@pytest.mark.parametrize("B,H,W", [(2, 6, 10), (3, 7, 5), (1, 9, 4)])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("epi,pre,cin2", EPIS)
def test_blocked_layouts(epi, pre, cin2, stride, B, H, W, cout):
    """Every CONVS_BLK_* bit alone and the combinations plan_layouts produces, against float64 and
    bitwise against blk = 0, on non-square maps with ragged pixel blocks (M = 120, 105, 36 at
    stride 1; 15, 12, 10 ... at stride 2)."""
    cin = 32 if cout == 48 else 64
    n = _layout_sweep((B, H, W, cin, cout, stride, cin2, epi), pre, seed=1000 + 10 * epi + stride + H)
    assert n == (5 if cin2 or epi in (2, 3) else 3)  # distinct layouts of the tensors the launch has


@pytest.mark.parametrize("cout", [48, 128])
def test_blocked_residual_of_an_odd_map(cout):
    """Epi 3 at stride 2 on a 15 x 10 map: the residual has res_H * res_W = 150 pixels per image and
    channel block, the output Ho * Wo = 40, and 2 oy reaches row 14 of 15."""
    n = _layout_sweep((2, 15, 10, 32, cout, 2, 0, 3), False, seed=1100,
                      layouts=[CONVS_BLK_RES, CONVS_BLK_RES | CONVS_BLK_Y, 15])
    assert n == 3


def _ulp_apart(a, b):
    """|a - b| in units of the larger float32 spacing at a / b (numpy f32 arrays)."""
    sp = np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b)))
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp


@pytest.mark.parametrize("blk", [0, CONVS_BLK_Y])
@pytest.mark.parametrize("epi,pre,cin2,stride", [(0, False, 32, 2), (2, False, 0, 1), (3, False, 0, 2),
                                                 (1, True, 0, 1), (1, False, 0, 1)])
def test_second_output_y2(epi, pre, cin2, stride, blk):
    """ConvParams::y2 = y * s2 + t2 beside y (epi 0, 2, 3 as run_conv launches it, and epi 1, which
    launch_convs accepts), NHWC and blocked (y2 follows y): y is bitwise the launch without y2; y2
    meets the bar against float64 ref * s2 + t2, and is within 1 float32 ulp of
    float32(double(y) * s2 + t2) from the returned y (the kernel's one fma rounds once, the host
    emulation twice).  Then the chain: conv1 without pre-BN on y2 is bitwise conv1 with (s2, t2) as its
    pre-BN on y (same weights)."""
    B, H, W, cin, cout = 3, 7, 5, 32, 48
    shape = (B, H, W, cin, cout, stride, cin2, epi)
    t, ref = _case(*shape, pre, 1200 + epi)
    d = _dev(t)
    s2, t2 = _rand(cout, seed=1290, lo=0.5, hi=1.5), _rand(cout, seed=1291, lo=-0.2, hi=0.2)
    y_alone = _launch(d, shape, blk=blk)
    y, y2 = _launch(d, shape, blk=blk, y2=(s2.to(DEV), t2.to(DEV)))
    assert torch.equal(y, y_alone), "y changes when y2 is written"
    _close(y, ref)
    assert torch.isfinite(y2).all()
    _close(y2, ref * s2.double() + t2.double())
    emu = (y.double() * s2.double() + t2.double()).float()
    assert _ulp_apart(y2.numpy(), emu.numpy()).max() <= 1.0
    # the next block's conv1 (cout -> 32 channels, stride 1) on both forms of its input
    Ho, Wo = y.shape[1], y.shape[2]
    w1 = (_rand(32, 9 * cout, seed=1292) / (9 * cout) ** 0.5).to(DEV)
    post = (_rand(32, seed=1293, lo=0.5, hi=1.5).to(DEV), _rand(32, seed=1294, lo=-0.2, hi=0.2).to(DEV))
    al = _rand(32, seed=1295, lo=0.1, hi=0.4).to(DEV)
    xb = blk and CONVS_BLK_X  # conv1 reads the blocked y / y2 as its blocked x
    on_y2 = _frt.conv2d_small(y2.to(DEV), w1, B, Ho, Wo, cout, 32, post=post, prelu=al, epi=1, blk=xb)
    on_y = _frt.conv2d_small(y.to(DEV), w1, B, Ho, Wo, cout, 32, pre=(s2.to(DEV), t2.to(DEV)), post=post, prelu=al,
                             epi=1, blk=xb)
    torch.cuda.synchronize()
    assert torch.isfinite(on_y2).all()
    assert torch.equal(on_y2, on_y), "conv1 on y2 differs from conv1 with pre-BN on y"


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin2", [16, 64, 128, 256])
def test_fused_shortcut_widths(cin2, stride):
    """The fused 1x1 shortcut at 1 chunk (one wave, three idle), 4 (one per wave), 8 and 16 chunks (2
    and SCMAX = 4 per wave: k >= 1 has its own weights and input chunk), NHWC and blocked x2."""
    n = _layout_sweep((2, 6, 10, 32, 48, stride, cin2, 0), False, seed=1300 + cin2, layouts=[CONVS_BLK_X2])
    assert n == 1


@pytest.mark.parametrize("B,H,W,stride", [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 17, 1), (2, 6, 10, 2)])
@pytest.mark.parametrize("cin", [16, 32, 48, 80, 256])
def test_register_ring_fill_edges(cin, B, H, W, stride):
    """A wave owns 9 * ncc chunks of the CH = 12 in flight: cin 16 -> 9 on wave 0 and three idle waves
    (0 chunks), 32 / 48 -> 9 (< CH), 80 -> 18 on wave 0 and 9 elsewhere, 256 -> 36 = 3 CH.  On a 1 x 1
    map one pixel has eight of its nine taps outside; 1 x 17 is one full pixel block and one lane
    of the next.  With pre-BN (masked per chunk from the ring's meta word) and without."""
    for pre in (True, False):
        shape = (B, H, W, cin, 16, stride, 0, 1)
        t, ref = _case(*shape, pre, 1400 + cin)
        got = _launch(_dev(t), shape)
        assert got.shape == ref.shape
        _close(got, ref)


def _refusal(shape, use_pre, **change):
    """The launch of _case(*shape) with some arguments replaced raises and leaves y untouched."""
    t, _ = _case(*shape, use_pre, 1500)
    d = _dev(t)
    y2 = change.pop("y2", None)
    d.update(change)
    B, H, W, cin, cout, stride = shape[:6]
    out = torch.full((B, (H - 1) // stride + 1, (W - 1) // stride + 1, cout), float("nan"), device=DEV)
    with pytest.raises(REFUSED):
        _launch(d, shape, y2=y2, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused launch wrote to y"


def test_refusals():
    """What launch_convs refuses, through an entry point that checks none of it itself."""
    one = torch.ones(48, device=DEV)
    # pre-BN with epi 0
    t, _ = _case(1, 9, 4, 32, 48, 1, 0, 1, True, 1500)
    _refusal((1, 9, 4, 32, 48, 1, 0, 0), False, pre=_dev(t)["pre"])
    # a shortcut of 17 chunks (SCMAX * NWV = 16), and one without its input
    _refusal((1, 9, 4, 32, 48, 1, 272, 0), False)
    _refusal((1, 9, 4, 32, 48, 1, 64, 0), False, x2=None)
    # epi 2 without its residual
    _refusal((1, 9, 4, 32, 48, 1, 0, 2), False, res=None)
    # y2 without its scale
    _refusal((1, 9, 4, 32, 48, 1, 0, 2), False, y2=(None, one))
    # pre-BN with more channels than the kernel stages in LDS (MAXC = 512)
    _refusal((1, 2, 3, 528, 16, 1, 0, 1), True)
