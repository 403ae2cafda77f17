"""GPU tests of the 160-wide tile of the three implicit-GEMM units (csrc/pww_conv.hip, pww_conv_tail.hip, pww_concat.hip; tile_n = 160).

The loop, the K order, the split bounds and the epilogues are those of the 64-wide tile, so one output element sees the same MFMA sequence
at every width: the bar is torch.equal between tile_n = 160 and tile_n = 64 at the same split. Cout = 160 has no 64-wide tile (64 does not
divide it); its 64-wide result is that of the Cout = 320 problem whose first 160 output channels are this one's (weight rows, bias and
residual channels appended behind them), cut back to 160 channels -- an output channel's sum depends on no other channel's weights.
One case per storage type is also held to the fp64 convolution of the rounded inputs at the bar of tests/test_conv_gpu.py.

Shapes: B H W = 128 (2 x 8 x 8: one full tile of rows) and 35 (1 x 5 x 7: the M tail), Cin 64 and 128 (9 and 18 K-slabs), Cout 160 (one
tile column) and 320 (two); stride 1 and 2, the fused upsample, with and without bias and residual; splitk 0 (the library's choice), 1, 2
and 5 (uneven: 5 divides neither 9 nor 18, and with the shortcut's slabs neither 10 .. 21).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float16]
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
SIZES = [(2, 8, 8), (1, 5, 7)]
SPLITS = (0, 1, 2, 5)
_ids = lambda v: str(v).split(".")[-1]  # noqa: E731


def _ops():
    from pww_hip import ops
    return ops


def _cl(t, dtype):
    return t.to(dtype).to(DEV).contiguous(memory_format=CL)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype and got.is_contiguous(memory_format=CL), what
    bad = got != want
    assert not bad.any(), "%s: %d of %d differ from the 64-wide tile, first at %s" % (what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())


def _split_of(lib_call, desc, M, Cout):
    """the split the library plans for this descriptor (from its workspace query): splitk = 0 must meet the 64-wide tile at the SAME split"""
    nbytes = int(lib_call(ctypes.byref(desc)))
    return nbytes // (4 * M * Cout) if nbytes else 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("Cout", [160, 320])
@pytest.mark.parametrize("Cin", [64, 128])
def test_conv3x3_equals_the_64_wide_tile(Cin, Cout, dtype):
    from pww_hip import _lib
    ops = _ops()
    g = torch.Generator().manual_seed(Cin + Cout)
    lib = _lib.load()
    for B, H, W in SIZES:
        x = _cl(torch.randn(B, Cin, H, W, generator=g), dtype)
        w320 = _cl(torch.randn(320, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5), dtype)
        b320 = (0.3 * torch.randn(320, generator=g)).to(dtype).to(DEV)
        for stride, up in ((1, False), (2, False), (1, True)):
            Ho, Wo = ((H << up) - 1) // stride + 1, ((W << up) - 1) // stride + 1
            r320 = _cl(torch.randn(B, 320, Ho, Wo, generator=g), dtype)
            w = w320[:Cout].contiguous(memory_format=CL)
            for bias, res in ((None, None), (b320, None), (b320, r320)):
                b = None if bias is None else bias[:Cout].contiguous()
                r = None if res is None else res[:, :Cout].contiguous(memory_format=CL)
                for splitk in SPLITS:
                    what = "conv3x3 %s %dx%dx%d %d -> %d stride %d up %d bias %s residual %s split %d" % (
                        dtype, B, H, W, Cin, Cout, stride, up, b is not None, r is not None, splitk)
                    got = ops.conv3x3(x, w, b, r, stride=stride, upsample=up, tile_n=160, splitk=splitk)
                    sk = splitk
                    if sk == 0:
                        d = _lib.ConvDesc(ctypes.sizeof(_lib.ConvDesc), ops._DT[dtype], B, H, W, Cin, Cout, stride, int(up), 160, 0, 0)
                        sk = _split_of(lib.pww_conv3x3_workspace_bytes, d, B * Ho * Wo, Cout)
                        assert sk >= 1, what
                    want = ops.conv3x3(x, w320, bias, res, stride=stride, upsample=up, tile_n=64, splitk=sk)[:, :Cout].contiguous(memory_format=CL)
                    _same(got, want, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_conv3x3_against_fp64(dtype):
    """fp64 convolution of the rounded inputs; the bar of tests/test_conv_gpu.py: |y - ref| <= 2 ULP (s + 1e-2 max s), s = |conv| + |conv + bias|
    (the convolution is rounded before the bias is added)."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    B, H, W, Cin, Cout = 1, 5, 7, 128, 320
    xc, wc = torch.randn(B, Cin, H, W, generator=g).to(dtype), (torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)).to(dtype)
    bc = (0.3 * torch.randn(Cout, generator=g)).to(dtype)
    conv = F.conv2d(xc.double(), wc.double(), None, 1, 1)
    ref = conv + bc.double()[None, :, None, None]
    scale = conv.abs() + ref.abs()
    tol = 2 * ULP[dtype] * (scale + 1e-2 * scale.max())
    for splitk in (1, 5):
        y = ops.conv3x3(_cl(xc, dtype), _cl(wc, dtype), bc.to(DEV), tile_n=160, splitk=splitk).cpu().double()
        err = (y - ref).abs()
        print("conv3x3 tile 160 %s split %d: max |err| %.3e, max |ref| %.3e, smallest margin %.3e" % (dtype, splitk, err.max().item(), ref.abs().max().item(),
                                                                                                     (tol - err).min().item()))
        assert not (err > tol).any(), "%d of %d outside the bar; max |err| %.3e" % (int((err > tol).sum()), err.numel(), err.max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("Cout", [160, 320])
@pytest.mark.parametrize("Cin", [64, 128])
def test_conv3x3_shortcut_equals_the_64_wide_tile(Cin, Cout, dtype):
    from pww_hip import _lib
    ops = _ops()
    g = torch.Generator().manual_seed(2 * Cin + Cout)
    lib = _lib.load_convtail()
    for B, H, W in SIZES:
        for C2 in (64, 192):
            h = _cl(torch.randn(B, Cin, H, W, generator=g), dtype)
            x = _cl(torch.randn(B, C2, H, W, generator=g), dtype)
            w320 = _cl(torch.randn(320, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5), dtype)
            s320 = (torch.randn(320, C2, 1, 1, generator=g) / C2 ** 0.5).to(dtype).to(DEV)
            b320, c320 = ((0.3 * torch.randn(320, generator=g)).to(dtype).to(DEV) for _ in range(2))
            w, s, b, c = w320[:Cout].contiguous(memory_format=CL), s320[:Cout].contiguous(), b320[:Cout].contiguous(), c320[:Cout].contiguous()
            for splitk in SPLITS:
                what = "conv3x3_shortcut %s %dx%dx%d %d + %d -> %d split %d" % (dtype, B, H, W, Cin, C2, Cout, splitk)
                got = ops.conv3x3_shortcut(h, w, b, x, s, c, tile_n=160, splitk=splitk)
                sk = splitk
                if sk == 0:
                    d = _lib.ConvTailDesc(ctypes.sizeof(_lib.ConvTailDesc), ops._DT[dtype], B, H, W, Cin, C2, Cout, 160, 0)
                    sk = _split_of(lib.pww_convtail_workspace_bytes, d, B * H * W, Cout)
                want = ops.conv3x3_shortcut(h, w320, b320, x, s320, c320, tile_n=64, splitk=sk)[:, :Cout].contiguous(memory_format=CL)
                _same(got, want, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("Cout", [160, 320])
@pytest.mark.parametrize("Cin", [64, 128])
def test_conv3x3_shortcut_cat_equals_the_64_wide_tile(Cin, Cout, dtype):
    from pww_hip import _lib
    ops = _ops()
    g = torch.Generator().manual_seed(3 * Cin + Cout)
    lib = _lib.load_concat()
    for B, H, W in SIZES:
        for C1, C2 in ((64, 128), (128, 64)):
            h = _cl(torch.randn(B, Cin, H, W, generator=g), dtype)
            x1, x2 = _cl(torch.randn(B, C1, H, W, generator=g), dtype), _cl(torch.randn(B, C2, H, W, generator=g), dtype)
            w320 = _cl(torch.randn(320, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5), dtype)
            s320 = (torch.randn(320, C1 + C2, 1, 1, generator=g) / (C1 + C2) ** 0.5).to(dtype).to(DEV)
            b320, c320 = ((0.3 * torch.randn(320, generator=g)).to(dtype).to(DEV) for _ in range(2))
            w, s, b, c = w320[:Cout].contiguous(memory_format=CL), s320[:Cout].contiguous(), b320[:Cout].contiguous(), c320[:Cout].contiguous()
            for splitk in SPLITS:
                what = "conv3x3_shortcut_cat %s %dx%dx%d %d + (%d, %d) -> %d split %d" % (dtype, B, H, W, Cin, C1, C2, Cout, splitk)
                got = ops.conv3x3_shortcut_cat(h, w, b, x1, x2, s, c, tile_n=160, splitk=splitk)
                sk = splitk
                if sk == 0:
                    d = _lib.ConcatTailDesc(ctypes.sizeof(_lib.ConcatTailDesc), ops._DT[dtype], B, H, W, Cin, C1, C2, Cout, 160, 0, 0)
                    sk = _split_of(lib.pww_concat_convtail_workspace_bytes, d, B * H * W, Cout)
                want = ops.conv3x3_shortcut_cat(h, w320, b320, x1, x2, s320, c320, tile_n=64, splitk=sk)[:, :Cout].contiguous(memory_format=CL)
                _same(got, want, what)


def test_tile_160_that_does_not_divide_cout_is_refused():
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    h = _cl(torch.randn(2, 64, 8, 8, generator=g), torch.bfloat16)
    w = _cl(torch.randn(128, 64, 3, 3, generator=g), torch.bfloat16)
    s = torch.randn(128, 64, 1, 1, generator=g).to(torch.bfloat16).to(DEV)
    b = torch.zeros(128, dtype=torch.bfloat16, device=DEV)
    for call in (lambda: ops.conv3x3(h, w, tile_n=160), lambda: ops.conv3x3_shortcut(h, w, b, h, s, b, tile_n=160),
                 lambda: ops.conv3x3_shortcut_cat(h, w, b, h[:, :64], h[:, :64], torch.cat([s, s], 1), b, tile_n=160)):
        with pytest.raises(ops.PwwHipError, match="tile_n 160 does not divide Cout 128"):
            call()
    assert torch.equal(ops.conv3x3(h, w, tile_n=128), ops.conv3x3(h, w, tile_n=64))
