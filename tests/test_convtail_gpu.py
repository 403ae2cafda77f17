"""GPU tests of pww_convtail_fwd (csrc/pww_conv_tail.hip: conv2 of a ResnetBlock2D with the block's 1 x 1 shortcut as further K-slabs of
the same implicit GEMM) and of its route in pww_hip/blocks.py.

Reference = an fp64 evaluation of the same (rounded) inputs on the CPU, computed once per input set and shared by every tile width and
split that runs on it.
* Small-integer (dyadic) inputs: every product and every partial sum is exact in fp32, so the kernel's one rounding of the exact sum must
  EQUAL the fp64 result rounded to the storage type -- for every tile width, every split, and wherever a split boundary falls.
* Random inputs: the fused form rounds once where the unfused sequence (ops.conv3x3 with the stock 1 x 1 GEMM as its residual) rounds four
  times, so its largest error may not exceed the unfused sequence's largest error on the same inputs by more than one rounding step of
  the storage type at the output's magnitude (ULP x max |ref|: what a tie may cost).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float16]
# (B, H, W): M = 128, one tile that spans two images; M = 35, a tile with clamped tail rows
SIZES = [(2, 8, 8), (1, 5, 7)]
CIN = 64
# (Cout, tile_n): both tile widths
TILES = [(64, 64), (128, 64), (128, 128)]
# Set by the issue: 1, 2, 5 on 9 + 3 slabs (5: two or three slabs per split, the drain path alone). Added here: 7 starts a split at slab 10,
# INSIDE the tail (12 k / 7 = 0 1 3 5 6 8 10), and 12 gives every slab a workgroup of its own.
SPLITS = [1, 2, 5, 7, 12]


def _ops():
    from pww_hip import ops
    return ops


def _ref64(h, w, b, x, w2, b2):
    """fp64 on the CPU: conv3x3(h, w) + conv1x1(x, w2) + b + b2, as a channels-first tensor"""
    h, w, b, x, w2, b2 = (t.detach().cpu().double() for t in (h, w, b, x, w2, b2))
    return F.conv2d(h.contiguous(), w.contiguous(), None, 1, 1) + F.conv2d(x.contiguous(), w2.contiguous()) + (b + b2)[None, :, None, None]


def _dyadic(size, C2, Cout, dtype, seed):
    """Small integers over a power of two: sums of up to 9 * 64 + 192 products stay far below 2^24 quarter-units -- exact in fp32."""
    B, H, W = size
    g = torch.Generator().manual_seed(seed)
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
    h = (ri((B, CIN, H, W), -3, 3) / 2).to(dtype).to(DEV).contiguous(memory_format=CL)
    x = (ri((B, C2, H, W), -3, 3) / 2).to(dtype).to(DEV).contiguous(memory_format=CL)
    w = (ri((Cout, CIN, 3, 3), -2, 2) / 2).to(dtype).to(DEV).contiguous(memory_format=CL)
    w2 = (ri((Cout, C2, 1, 1), -2, 2) / 2).to(dtype).to(DEV)
    b, b2 = (ri((Cout,), -8, 8) / 4).to(dtype).to(DEV), (ri((Cout,), -8, 8) / 4).to(dtype).to(DEV)
    return h, w, b, x, w2, b2


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("size", SIZES, ids=["2x8x8", "1x5x7"])
@pytest.mark.parametrize("C2", [64, 192])
def test_dyadic_inputs_equal_fp64_for_every_tile_and_split(dtype, size, C2):
    ops = _ops()
    for Cout in (64, 128):
        t = _dyadic(size, C2, Cout, dtype, seed=C2 + Cout)
        want = _ref64(*t).to(dtype)                    # (the exact sum, rounded once)
        assert want.float().abs().max() > 8            # (the sums are not trivially small)
        for tile_n in [tn for co, tn in TILES if co == Cout]:
            for splitk in [s for s in SPLITS if s <= 9 + C2 // 64]:
                y = ops.conv3x3_shortcut(*t, tile_n=tile_n, splitk=splitk)
                assert y.shape == want.shape and y.dtype == dtype and y.is_contiguous(memory_format=CL)
                bad = (y.cpu() != want)
                assert not bad.any(), "Cout %d tile_n %d splitk %d: %d of %d differ, first at %s" % (
                    Cout, tile_n, splitk, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
        # the library's own choice of tile and split
        assert torch.equal(ops.conv3x3_shortcut(*t).cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("size", SIZES, ids=["2x8x8", "1x5x7"])
def test_probe_one_corner_pixel_through_a_one_hot_shortcut(dtype, size):
    """h = 0, x = 0 but one corner pixel, w2 one-hot: the output is nonzero at that pixel and that channel only -- the tail reads the centre
    tap (no halo, no neighbour) with row pitch C2 and weight row n C2."""
    ops = _ops()
    B, H, W = size
    C2, Cout = 192, 128
    g = torch.Generator().manual_seed(3)
    w = torch.randn(Cout, CIN, 3, 3, generator=g).to(dtype).to(DEV).contiguous(memory_format=CL)
    h = torch.zeros(B, CIN, H, W, dtype=dtype, device=DEV).contiguous(memory_format=CL)
    zero = torch.zeros(Cout, dtype=dtype, device=DEV)
    for (pb, py, px), c0, n0 in (((0, 0, 0), 0, 0), ((B - 1, H - 1, W - 1), C2 - 1, Cout - 1), ((B - 1, 0, W - 1), 70, 65), ((0, H - 1, 0), 129, 3)):
        x = torch.zeros(B, C2, H, W, dtype=dtype, device=DEV).contiguous(memory_format=CL)
        x[pb, c0, py, px] = 3.0
        x[pb, (c0 + 1) % C2, py, px] = 5.0                     # (a neighbouring channel the one-hot weight must not pick up)
        w2 = torch.zeros(Cout, C2, 1, 1, dtype=dtype, device=DEV)
        w2[n0, c0] = 0.5
        want = torch.zeros(B, Cout, H, W, dtype=dtype)
        want[pb, n0, py, px] = 1.5
        for tile_n, splitk in ((64, 1), (128, 1), (128, 7), (64, 12)):
            y = ops.conv3x3_shortcut(h, w, zero, x, w2, zero, tile_n=tile_n, splitk=splitk).cpu()
            assert torch.equal(y, want), ((pb, py, px), c0, n0, tile_n, splitk, y.nonzero().tolist()[:8])


def _random(size, C2, Cout, dtype, seed):
    B, H, W = size
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, CIN, H, W, generator=g).to(dtype).to(DEV).contiguous(memory_format=CL)
    x = torch.randn(B, C2, H, W, generator=g).to(dtype).to(DEV).contiguous(memory_format=CL)
    w = (torch.randn(Cout, CIN, 3, 3, generator=g) / (3 * CIN ** 0.5)).to(dtype).to(DEV).contiguous(memory_format=CL)
    w2 = (torch.randn(Cout, C2, 1, 1, generator=g) / C2 ** 0.5).to(dtype).to(DEV)
    b, b2 = (torch.randn(Cout, generator=g) * 0.3).to(dtype).to(DEV), (torch.randn(Cout, generator=g) * 0.3).to(dtype).to(DEV)
    return h, w, b, x, w2, b2


def _unfused(ops, h, w, b, x, w2, b2):
    """The parent route: the 1 x 1 shortcut as a stock GEMM with its bias over the [B H W, C] view, then conv2 with bias and residual."""
    B, C2, H, W = x.shape
    Cout = w.shape[0]
    r = F.linear(x.permute(0, 2, 3, 1).reshape(B * H * W, C2), w2.reshape(Cout, C2), b2).view(B, H, W, Cout).permute(0, 3, 1, 2)
    return ops.conv3x3(h, w, b, residual=r)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("size", SIZES, ids=["2x8x8", "1x5x7"])
@pytest.mark.parametrize("C2", [64, 192])
def test_random_inputs_no_worse_than_the_unfused_sequence(dtype, size, C2):
    ops = _ops()
    for Cout in (64, 128):
        t = _random(size, C2, Cout, dtype, seed=7 + C2 + Cout)
        ref = _ref64(*t)
        step = ULP[dtype] * ref.abs().max().item()
        e_parent = (_unfused(ops, *t).cpu().double() - ref).abs().max().item()
        for tile_n in [tn for co, tn in TILES if co == Cout]:
            for splitk in (0, 1, 2, 5):
                e_fused = (ops.conv3x3_shortcut(*t, tile_n=tile_n, splitk=splitk).cpu().double() - ref).abs().max().item()
                print("convtail random %s %s C2 %d Cout %d tile_n %d splitk %d: max |err| fused %.4e, unfused %.4e, one step %.4e (max |ref| %.3f)"
                      % (str(dtype).split(".")[-1], size, C2, Cout, tile_n, splitk, e_fused, e_parent, step, ref.abs().max().item()))
                assert e_fused <= e_parent + step, (Cout, tile_n, splitk, e_fused, e_parent, step)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_resnet_block_with_the_route_on_and_off(dtype, monkeypatch):
    """One ResnetBlock2D of the stand-in (64 -> 128 channels, 8 x 8) through install_blocks against the module in fp64: the same bound, and
    the counter says which way each call went."""
    import pww_hip.blocks as blocks
    from sd_standin import unet as U
    torch.manual_seed(0)
    res = U.ResnetBlock2D(64, 128, 64, 32).to(dtype).eval()                 # (parameters rounded to the storage type first)
    x = torch.randn(2, 64, 8, 8).to(dtype)
    temb = torch.randn(2, 64).to(dtype)
    with torch.no_grad():
        ref = U.ResnetBlock2D(64, 128, 64, 32).double().eval()
        ref.load_state_dict({k: v.double() for k, v in res.state_dict().items()})
        want = ref(x.double(), temb.double())
        res = res.to(DEV).to(memory_format=CL)
        xd, td = x.to(DEV).contiguous(memory_format=CL), temb.to(DEV)
        blocks.install_blocks(res)
        try:
            out = {}
            for on in (False, True):
                monkeypatch.setattr(blocks, "CONV_SHORTCUT", on)
                blocks.reset_stats()
                out[on] = res(xd, td)
                st = blocks.stats()
                assert st["conv_shortcut"] == ({"fused": 1, "declined": 0} if on else {"fused": 0, "declined": 1}), st
                assert st["conv3x3"] == {"fused": 2, "declined": 0} and st["conv1x1"]["fused"] == (0 if on else 1) and st["hit_rate"] == 1.0, st
        finally:
            blocks.uninstall_blocks(res)
    step = ULP[dtype] * want.abs().max().item()
    e_off, e_on = ((out[k].cpu().double() - want).abs().max().item() for k in (False, True))
    print("convtail block %s: max |err| route on %.4e, off %.4e, one step %.4e" % (str(dtype).split(".")[-1], e_on, e_off, step))
    assert out[True].shape == want.shape and out[True].is_contiguous(memory_format=CL)
    assert e_on <= e_off + step, (e_on, e_off, step)


def test_more_splits_than_slabs_and_mismatched_operands_are_refused():
    ops = _ops()
    h, w, b, x, w2, b2 = _random((1, 5, 7), 64, 64, torch.bfloat16, seed=1)
    with pytest.raises(ops.PwwHipError, match="exceeds the 10 K-slabs"):
        ops.conv3x3_shortcut(h, w, b, x, w2, b2, splitk=11)
    assert not ops.conv3x3_shortcut_takes(h, w, x.contiguous(), w2)                       # NCHW shortcut input
    assert not ops.conv3x3_shortcut_takes(h, w, x[:, :, :4], w2)                          # another size
    assert not ops.conv3x3_shortcut_takes(h, w, x.half(), w2.half())                      # another dtype
    assert not ops.conv3x3_shortcut_takes(h, w, x[:, :32].contiguous(memory_format=CL), w2[:, :32].contiguous())      # C2 32: no slab
    with pytest.raises(ops.PwwHipError, match="shortcut_bias"):
        ops.conv3x3_shortcut(h, w, b, x, w2, b2[:32])
