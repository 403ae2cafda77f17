"""GPU tests of PWW_PARTIAL_STORES (csrc/pww_common.h: store_partial_through, partial_stores_through): the split-K launches of
ops.conv3x3, ops.conv3x3_shortcut, ops.conv3x3_shortcut_cat and ops.linear store their fp32 partials either with plain 16-byte stores or
write-through. The switch is read on the host at every call and moves no bit: the ONLY bar is torch.equal between the two, and a call
with the switch flipped back gives the first bits again.

Shapes: B H W = 128 (2 x 8 x 8: one full tile of 128 rows) and 35 (1 x 5 x 7: the M tail, rows a lane must not store), Cin 64 and 128,
Cout 160 (the 160-wide tile alone) and 320 (every tile width divides it or not: 64 and 160), split 2 and 5 (5 does not divide the 9 / 18
K-slabs: uneven splits). ops.linear: M = 128 and 35, N = 64 and 128, K = 256 at split 2 -- K = 256 is 4 K-slabs, so split 5 is refused there
(held below) and runs at K = 320, with split 2 beside it.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float16]
SIZES = [(2, 8, 8), (1, 5, 7)]
_ids = lambda v: str(v).split(".")[-1]  # noqa: E731


def _ops():
    from pww_hip import ops
    return ops


def _cl(t, dtype):
    return t.to(dtype).to(DEV).contiguous(memory_format=CL)


def _both_ways(monkeypatch, call, what):
    """plain, through, plain again: all three the same bits"""
    outs = []
    for mode in ("plain", "through", "plain", "through"):
        monkeypatch.setenv("PWW_PARTIAL_STORES", mode)
        outs.append(call())
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all(), what
    for mode, o in zip(("through", "plain again", "through again"), outs[1:]):
        bad = o != outs[0]
        assert not bad.any(), "%s, %s: %d of %d differ from the plain stores' result" % (what, mode, int(bad.sum()), bad.numel())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_conv3x3(dtype, monkeypatch):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    for B, H, W in SIZES:
        for Cin in (64, 128):
            for Cout in (160, 320):
                x = _cl(torch.randn(B, Cin, H, W, generator=g), dtype)
                w = _cl(torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5), dtype)
                b = (0.3 * torch.randn(Cout, generator=g)).to(dtype).to(DEV)
                r = _cl(torch.randn(B, Cout, H, W, generator=g), dtype)
                for splitk in (2, 5):
                    for tile_n in ((160,) if Cout == 160 else (64, 160)):
                        what = "conv3x3 %s %dx%dx%d %d -> %d tile %d split %d" % (dtype, B, H, W, Cin, Cout, tile_n, splitk)
                        _both_ways(monkeypatch, lambda: ops.conv3x3(x, w, b, r, tile_n=tile_n, splitk=splitk), what)
                    _both_ways(monkeypatch, lambda: ops.conv3x3(x, w, None, None, stride=2, splitk=splitk), "stride 2, " + what)
                    _both_ways(monkeypatch, lambda: ops.conv3x3(x, w, b, None, upsample=True, splitk=splitk), "upsample, " + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_conv3x3_shortcut(dtype, monkeypatch):
    ops = _ops()
    g = torch.Generator().manual_seed(4)
    for B, H, W in SIZES:
        for Cin, C2 in ((64, 192), (128, 64)):
            for Cout in (160, 320):
                h = _cl(torch.randn(B, Cin, H, W, generator=g), dtype)
                x = _cl(torch.randn(B, C2, H, W, generator=g), dtype)
                w = _cl(torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5), dtype)
                w2 = (torch.randn(Cout, C2, 1, 1, generator=g) / C2 ** 0.5).to(dtype).to(DEV)
                b, b2 = ((0.3 * torch.randn(Cout, generator=g)).to(dtype).to(DEV) for _ in range(2))
                for splitk in (2, 5):
                    for tile_n in ((160,) if Cout == 160 else (64, 160)):
                        what = "conv3x3_shortcut %s %dx%dx%d %d + %d -> %d tile %d split %d" % (dtype, B, H, W, Cin, C2, Cout, tile_n, splitk)
                        _both_ways(monkeypatch, lambda: ops.conv3x3_shortcut(h, w, b, x, w2, b2, tile_n=tile_n, splitk=splitk), what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_conv3x3_shortcut_cat(dtype, monkeypatch):
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    for B, H, W in SIZES:
        for Cin, (C1, C2) in ((64, (64, 128)), (128, (128, 64))):
            for Cout in (160, 320):
                h = _cl(torch.randn(B, Cin, H, W, generator=g), dtype)
                x1, x2 = _cl(torch.randn(B, C1, H, W, generator=g), dtype), _cl(torch.randn(B, C2, H, W, generator=g), dtype)
                w = _cl(torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5), dtype)
                w2 = (torch.randn(Cout, C1 + C2, 1, 1, generator=g) / (C1 + C2) ** 0.5).to(dtype).to(DEV)
                b, b2 = ((0.3 * torch.randn(Cout, generator=g)).to(dtype).to(DEV) for _ in range(2))
                for splitk in (2, 5):
                    for tile_n in ((160,) if Cout == 160 else (64, 160)):
                        what = "conv3x3_shortcut_cat %s %dx%dx%d %d + (%d, %d) -> %d tile %d split %d" % (dtype, B, H, W, Cin, C1, C2, Cout, tile_n, splitk)
                        _both_ways(monkeypatch, lambda: ops.conv3x3_shortcut_cat(h, w, b, x1, x2, w2, b2, tile_n=tile_n, splitk=splitk), what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_linear(dtype, monkeypatch):
    ops = _ops()
    g = torch.Generator().manual_seed(6)
    for M in (128, 35):
        for N in (64, 128):
            for K, splits in ((256, (2,)), (320, (2, 5))):
                x = torch.randn(M, K, generator=g).to(dtype).to(DEV)
                w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).to(DEV)
                b = (0.3 * torch.randn(N, generator=g)).to(dtype).to(DEV)
                r = torch.randn(M, N, generator=g).to(dtype).to(DEV)
                for splitk in splits:
                    for tile_n in ((64,) if N == 64 else (64, 128)):
                        what = "linear %s M %d N %d K %d tile %d split %d" % (dtype, M, N, K, tile_n, splitk)
                        _both_ways(monkeypatch, lambda: ops.linear(x, w, b, r, tile_n=tile_n, splitk=splitk), what)
                        _both_ways(monkeypatch, lambda: ops.linear(x, w, tile_n=tile_n, splitk=splitk), "no epilogue, " + what)
                    if N == 128:
                        _both_ways(monkeypatch, lambda: ops.linear(x, w, b, geglu=True, tile_n=128, splitk=splitk), "geglu, " + what)
                if K == 256:        # 4 K-slabs: no split 5, whatever the stores
                    with pytest.raises(ops.PwwHipError):
                        ops.linear(x, w, b, splitk=5)


def test_unknown_value_is_the_default(monkeypatch):
    """Anything but `plain` / `through` leaves the default: same bits again."""
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    x = _cl(torch.randn(2, 64, 8, 8, generator=g), torch.bfloat16)
    w = _cl(torch.randn(320, 64, 3, 3, generator=g) / 24, torch.bfloat16)
    monkeypatch.setenv("PWW_PARTIAL_STORES", "plain")
    want = ops.conv3x3(x, w, splitk=3)
    for v in ("", "1", "THROUGH"):
        monkeypatch.setenv("PWW_PARTIAL_STORES", v)
        assert torch.equal(ops.conv3x3(x, w, splitk=3), want)
    monkeypatch.delenv("PWW_PARTIAL_STORES")
    assert torch.equal(ops.conv3x3(x, w, splitk=3), want)
