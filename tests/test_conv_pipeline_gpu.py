"""GPU tests of the multi-stage K loop of pww_conv3x3_fwd (csrc/pww_conv.hip): the places where a loop that keeps several K-slabs of loads
in flight goes wrong are its prologue and its drain (fewer slabs than stages), the zero source of the padding halo and of the M tail, and
state carried from one call to the next.

Reference and bar as in test_conv_gpu.py, restated here: reference = fp32 F.conv2d of the same (rounded) inputs; bar = one rounding step of
the storage type relative to the output's spread, |y - ref| <= 2 ULP (s + 1e-2 max s), s = |ref| (+ |conv| with a bias: the conv is rounded
before the bias is added) -- fp32 accumulation, one rounding.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
CL = torch.channels_last


def _ops():
    from pww_hip import ops
    return ops


def _inputs(rows, Cin, Cout, Hin, Win, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, Cin, Hin, Win, device=DEV, generator=g).to(dtype).contiguous(memory_format=CL)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(dtype).contiguous(memory_format=CL)
    b = (torch.randn(Cout, device=DEV, generator=g) * 0.3).to(dtype)
    return x, w, b


def _reference(x, w, b, stride, up):
    xf = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
    conv = F.conv2d(xf, w.float(), None, stride, 1)
    if b is None:
        return conv, conv.abs()
    ref = conv + b.float()[None, :, None, None]
    return ref, conv.abs() + ref.abs()


def _check(y, ref_scale, dtype, steps=2):
    ref, scale = ref_scale
    assert y.shape == ref.shape and y.dtype == dtype
    assert y.is_contiguous(memory_format=CL)
    yf = y.float()
    tol = steps * ULP[dtype] * (scale + 1e-2 * scale.max())
    bad = (yf - ref).abs() > tol
    assert not bad.any(), "%d of %d outside the bar; max |err| %.3e (max |ref| %.3e)" % (int(bad.sum()), bad.numel(), (yf - ref).abs().max().item(),
                                                                                         ref.abs().max().item())


def _slabs_per_split(nslab, splitk):
    return [(k + 1) * nslab // splitk - k * nslab // splitk for k in range(splitk)]


def test_forced_splits_cover_one_to_four_slabs():
    """Cin = 64 is 9 K-slabs; the splits below give workgroups of 1, 2, 3 and 4 slabs (the kernel's own split rule, restated)."""
    seen = set()
    for sk in range(2, 10):
        seen.update(_slabs_per_split(9, sk))
    assert {1, 2, 3, 4} <= seen


@pytest.mark.parametrize("stride,up", [(1, 0), (2, 0), (1, 1)], ids=["s1", "s2", "up"])
@pytest.mark.parametrize("tile_n", [64, 128])
@pytest.mark.parametrize("splitk", list(range(2, 10)))
def test_short_k_per_workgroup(splitk, tile_n, stride, up):
    """fewer slabs per workgroup than the loop has stages: prologue and drain only"""
    ops = _ops()
    x, w, b = _inputs(2, 64, 128, 12, 10, torch.bfloat16, seed=10 + splitk)
    y = ops.conv3x3(x, w, b, stride=stride, upsample=bool(up), tile_n=tile_n, splitk=splitk)
    _check(y, _reference(x, w, b, stride, up), torch.bfloat16)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (63, 61)], ids=lambda v: str(v))
@pytest.mark.parametrize("stride,up", [(1, 0), (2, 0), (1, 1)], ids=["s1", "s2", "up"])
def test_halo_and_m_tail(H, W, stride, up):
    """every output pixel of the small maps touches the halo; 3 x H x W is never a multiple of the 128-row tile"""
    ops = _ops()
    x, w, b = _inputs(3, 128, 128, H, W, torch.bfloat16, seed=20)
    y = ops.conv3x3(x, w, b, stride=stride, upsample=bool(up))
    _check(y, _reference(x, w, b, stride, up), torch.bfloat16)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (63, 61)], ids=lambda v: str(v))
def test_no_state_carried_between_calls(H, W):
    """the same call before and after a call on a different shape (another Cin, tile width, split and map size): bitwise the same, and right"""
    ops = _ops()
    x, w, b = _inputs(3, 128, 128, H, W, torch.bfloat16, seed=21)
    first = ops.conv3x3(x, w, b)
    x2, w2, b2 = _inputs(2, 320, 192, 9, 14, torch.bfloat16, seed=22)
    other = ops.conv3x3(x2, w2, b2, tile_n=64, splitk=5)
    _check(other, _reference(x2, w2, b2, 1, 0), torch.bfloat16)
    again = ops.conv3x3(x, w, b)
    assert torch.equal(first, again)
    _check(again, _reference(x, w, b, 1, 0), torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("Cin,Cout,S,splitk", [(64, 128, 12, 4), (320, 320, 16, 7), (640, 1280, 8, 12), (1280, 1280, 8, 24)])
def test_split_agrees_with_unsplit_and_repeats(Cin, Cout, S, splitk, dtype):
    """split s and split 1 of the same input: each within the bar of the fp32 reference and within the bar of each other (the fp32 sums
    differ in their last bits, so a rounding of the conv and one of conv + bias may each flip by one step: 2^-7 (|conv| + |ref|) in bf16,
    half the bar), and each bitwise equal to itself over three calls"""
    ops = _ops()
    x, w, b = _inputs(2, Cin, Cout, S, S, dtype, seed=30)
    ref = _reference(x, w, b, 1, 0)
    outs = {}
    for sk in (1, splitk):
        ys = [ops.conv3x3(x, w, b, splitk=sk) for _ in range(3)]
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
        _check(ys[0], ref, dtype)
        outs[sk] = ys[0].float()
    scale = ref[1]
    tol = 2 * ULP[dtype] * (scale + 1e-2 * scale.max())
    assert not ((outs[1] - outs[splitk]).abs() > tol).any()
