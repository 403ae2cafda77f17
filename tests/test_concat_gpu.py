"""GPU tests of libpww_hip_concat.so (csrc/pww_concat.hip): GroupNorm and conv2 + shortcut reading the two halves of
`torch.cat([x1, x2], 1)` where they lie, and the restated up block of pww_hip/blocks.py.

The bar is torch.equal against the existing one-source op on the concatenated tensor: a concatenation copies and computes nothing,
and the two-source kernels keep launch form, summation order, tile, K order and split of the one-source ones. One float16 GroupNorm case
under a large mean is also held to norm_cases.reference: equality alone would not see a mistake that both copies of the kernels share.

GroupNorm shapes. The launch form is chosen by shape (the two-source op asks the same selector for C1 + C2 channels), so each form is
reached the way test_norm_edges_gpu.py reaches it, by a shape, and the form is asserted from the workspace size (16 bytes: one launch):
  (64, 32, 8)      cg = 12: group 5 holds channels 60 .. 71 and straddles the boundary, an 8-channel chunk spans two groups. One launch at
                   8 x 8, 5 x 8 (tail pixels, fewer pixels than the 85 in flight) and 16 x 16; 48 x 48 is past the 24 pieces a thread holds:
                   the two-launch form at 256 threads, straddling.
  (64, 32, 16)     cg = 6 is no multiple of 4: the two-launch form at every size, slabs shorter than one trip, group 10 straddles.
  (64, 64, 32), (8, 24, 4)     boundary on a group edge; 4-channel pieces right at the boundary.
  (1280, 1280, 32), (1288, 1272, 32)  at 24 x 24: C > 2048 and more than 24 pieces, the 512-thread two-launch form; the second pair puts
                   the boundary inside group 16 and off the 64-channel grid.
5 x 7 (HW no multiple of 8) and 2 x 2 (HW = 4) are shapes the one-source op refuses (`HW % 8`, `HW >= 8` in its plan); the two-source op
follows it, and the test holds both to the refusal. 5 x 8 carries the tail-pixel case instead.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float16]
_ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v).split(".")[-1]  # noqa: E731


def _ops():
    from pww_hip import ops
    return ops


def _cl(t, dtype):
    return t.to(dtype).to(DEV).contiguous(memory_format=CL)


# (C1, C2, groups): [(H, W, form)]; form "group" = one launch, 256 / 512 = threads of the two-launch form
GN_CASES = {
    (64, 32, 8): [(8, 8, "group"), (5, 8, "group"), (16, 16, "group"), (48, 48, 256)],
    (64, 32, 16): [(8, 8, 256), (5, 8, 256), (16, 16, 256)],
    (64, 64, 32): [(8, 8, "group"), (5, 8, "group"), (16, 16, "group")],
    (8, 24, 4): [(8, 8, "group"), (5, 8, "group"), (16, 16, "group")],
    (1280, 1280, 32): [(24, 24, 512)],
    (1288, 1272, 32): [(24, 24, 512)],
}


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", list(GN_CASES), ids=_ids)
def test_group_norm_equals_the_one_source_op_on_the_concatenation(case, dtype):
    from pww_hip import _lib
    ops = _ops()
    C1, C2, G = case
    C, B = C1 + C2, 2
    g = torch.Generator().manual_seed(C1 + 7 * C2 + G)
    w, b = (1 + 0.3 * torch.randn(C, generator=g)).to(dtype).to(DEV), (0.3 * torch.randn(C, generator=g)).to(dtype).to(DEV)
    for H, W, form in GN_CASES[case]:
        # a mean and a spread per channel: a wrong source, pitch or channel offset moves whole groups
        mean, spread = 2 * torch.randn(1, C, 1, 1, generator=g), 0.5 + torch.rand(1, C, 1, 1, generator=g)
        x = mean + spread * torch.randn(B, C, H, W, generator=g)
        x1, x2 = _cl(x[:, :C1], dtype), _cl(x[:, C1:], dtype)
        cat = torch.cat([x1, x2], dim=1).contiguous(memory_format=CL)
        need = int(_lib.load_concat().pww_concat_group_norm_workspace_bytes(ctypes.byref(ops._gn_cat_desc(x1, x2, G, 1e-5, None))))
        nslab = {(48, 48): 14, (8, 8): 1, (5, 8): 1, (16, 16): 2, (24, 24): 64}[(H, W)]
        assert need == (16 if form == "group" else B * nslab * G * 16), (case, H, W, need)                  # the form this shape was picked for
        assert (C // 8 > 256) == (form == 512)
        for act in (None, "silu"):
            for ww, bb in ((w, b), (None, None)):
                want = ops.group_norm(cat, G, ww, bb, 1e-5, act=act)
                got = ops.group_norm_cat(x1, x2, G, ww, bb, 1e-5, act=act)
                assert got.shape == want.shape and got.dtype == dtype and got.is_contiguous(memory_format=CL)
                bad = got != want
                assert not bad.any(), "%s %dx%d act %s affine %s: %d of %d differ, first at %s" % (
                    case, H, W, act, ww is not None, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
        # a caller's workspace full of 0xFF (NaN partials wherever a kernel reads what it did not write): the same bits
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        assert torch.equal(ops.group_norm_cat(x1, x2, G, w, b, 1e-5, act="silu", workspace=ws), ops.group_norm(cat, G, w, b, 1e-5, act="silu"))


# float16 under a large mean, the smallest shape of each launch form above: (C1, C2, groups) -> (H, W, form, nslab)
STAT_CASES = {(64, 32, 8): (8, 8, "group", 1), (64, 32, 16): (16, 16, 256, 2), (1280, 1280, 32): (24, 24, 512, 64)}


@pytest.mark.parametrize("case", list(STAT_CASES), ids=_ids)
def test_group_norm_float16_statistics_under_a_large_mean(case):
    """Every channel at mean 300 with a spread of 0.5, float16: where plain fp32 sums of float16 squares break (csrc/pww_norm.hip, header),
    so the pivot of the two-source kernels -- in the two-launch forms handed to the fold through LDS -- has to be right. Two bars:
      * torch.equal with ops.group_norm on the concatenation: this unit's own source select and pitch in front of the first load;
      * norm_cases.reference (fp64 statistics, the kernel's rounding points): one rounding step, two behind SiLU, no element outside. The
        kernels of csrc/pww_concat.hip are a copy of those of csrc/pww_norm.hip, and test_norm_edges_gpu.py holds the one-source op to the
        reference under this mean at other shapes only: equality alone would pass a mistake both copies share at these.
    No affine map and eps 1e-6, as in test_norm_edges_gpu.py's large-mean test: the output is (h - mean) * rstd, and the reference's own
    fp32 `h * a + b` then rounds once at magnitude 600 (half a unit there, 3.1e-5, plus half a float16 spacing of the result, against the
    bar's floor of 2^-10 * 1e-2 * max |ref| = 3.9e-5 at max |ref| = 4.0); with gamma and beta its b takes two more roundings of that size
    and the reference would be looser than the bar.
    On the CPU, at these inputs: the reference is finite (max |ref| 4.0 - 5.0). The stock sequence is within the bars behind SiLU (worst
    0.62 - 0.86 of the tolerance) and NOT in front of it: with the norm in fp32 609 of 12 288, 1 853 of 49 152 and 163 127 of 2 949 120
    elements lie outside one step (worst 1.8 - 2.0 tolerances), with the norm in fp64 still 0, 1 233 and 26 934 (worst 0.9 - 1.7), every one
    of them at |ref| < 0.05, where the bar is its floor (3.9e-5) and every fp32 rounding at this mean is of the floor's size: the stock
    op's fp32 statistics, and the fp32 mean (300) and b = -a * mean (600) that the reference shares with the kernels but not with the
    stock op. So the stock sequence is no yardstick for outputs near zero in this regime; the bar against the reference stands as set."""
    import norm_cases as N
    from pww_hip import _lib
    ops = _ops()
    dtype = torch.float16
    C1, C2, G = case
    H, W, form, nslab = STAT_CASES[case]
    C, B = C1 + C2, 2
    g = torch.Generator().manual_seed(11 + C1 + 7 * C2 + G)
    x = 300.0 + 0.5 * torch.randn(B, C, H, W, generator=g)
    x1, x2 = _cl(x[:, :C1], dtype), _cl(x[:, C1:], dtype)
    cat = torch.cat([x1, x2], dim=1).contiguous(memory_format=CL)
    need = int(_lib.load_concat().pww_concat_group_norm_workspace_bytes(ctypes.byref(ops._gn_cat_desc(x1, x2, G, 1e-6, None))))
    assert need == (16 if form == "group" else B * nslab * G * 16) and (C // 8 > 256) == (form == 512), (case, need)
    for act in (None, "silu"):
        got = ops.group_norm_cat(x1, x2, G, None, None, 1e-6, act=act)
        want = ops.group_norm(cat, G, None, None, 1e-6, act=act)
        ref = N.reference(cat, None, None, None, G, 1e-6, act, dtype)
        nbad, rel = N.close(got, ref, dtype, steps=2 if act else 1)
        print("large mean %s %dx%d %s act %s: equal %s, %d outside, max |diff| / max |ref| %.3e" % (case, H, W, form, act, torch.equal(got, want), nbad, rel))
        assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 1.0
        assert torch.equal(got, want), (case, act, int((got != want).sum()))
        assert nbad == 0, (case, act, nbad, rel)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_group_norm_follows_the_one_source_op_where_it_refuses(dtype):
    """5 x 7 (HW = 35) and 2 x 2 (HW = 4): pww_group_norm_fwd takes neither, so neither does the two-source op, and both say so."""
    ops = _ops()
    for (C1, C2, G), (H, W) in (((64, 32, 8), (5, 7)), ((64, 64, 32), (5, 7)), ((8, 24, 4), (5, 7)), ((1280, 1280, 32), (2, 2))):
        x1, x2 = _cl(torch.randn(2, C1, H, W), dtype), _cl(torch.randn(2, C2, H, W), dtype)
        assert not ops.group_norm_cat_takes(x1, x2, G)
        with pytest.raises(ops.PwwHipError):
            ops.group_norm(torch.cat([x1, x2], dim=1).contiguous(memory_format=CL), G)
        with pytest.raises(ops.PwwHipError):
            ops.group_norm_cat(x1, x2, G)


def test_group_norm_declines_what_the_kernels_do_not_take():
    ops = _ops()
    x1, x2 = _cl(torch.randn(2, 64, 8, 8), torch.bfloat16), _cl(torch.randn(2, 32, 8, 8), torch.bfloat16)
    assert ops.group_norm_cat_takes(x1, x2, 8)
    assert not ops.group_norm_cat_takes(x1.contiguous(), x2, 8)                       # NCHW
    assert not ops.group_norm_cat_takes(x1, x2.half(), 8)                             # two dtypes
    assert not ops.group_norm_cat_takes(x1, x2[:, :, :4], 8)                          # two sizes
    assert not ops.group_norm_cat_takes(x1[:, :60].contiguous(memory_format=CL), x2, 4)      # a part off the 8-channel grid
    assert not ops.group_norm_cat_takes(x1, x2, 7)                                    # groups that do not divide
    assert not ops.group_norm_cat_takes(x1.cpu(), x2.cpu(), 8)
    assert not ops.group_norm_cat_takes(x1, x2, 8, weight=torch.ones(96, device=DEV))                 # fp32 affine parameters
    with pytest.raises(ops.PwwHipError, match="act"):
        ops.group_norm_cat(x1, x2, 8, act="gelu")


# ---- conv2 + shortcut ---------------------------------------------------------------------------------------------------------------------
SIZES = [(2, 8, 8), (1, 5, 7)]           # M = 128: one tile that spans two images; M = 35: a tile with clamped tail rows
CMID = 64
PARTS = [(64, 128), (128, 64), (64, 64)]
TILES = [(64, 64), (128, 64), (128, 128)]          # (Cout, tile_n): both tile widths


def _splits(C1, C2):
    """Set by the issue: 0, 1, 2, 5. K runs over 9 slabs of the gather, C1 / 64 of x1, C2 / 64 of x2. With one workgroup per slab (split =
    the slab count) a split starts at EVERY slab: inside x1, on the first slab of x2 and inside x2 where they have more than one slab; 7 puts
    boundaries at slabs 1, 3, 5, 6, 8, 10 of 12 -- the second slab of the tail, which is x2's first for (64, 128) and x1's second for (128, 64)."""
    n = 9 + (C1 + C2) // 64
    return [0, 1, 2, 5, 7, n]


def _tail_inputs(size, C1, C2, Cout, dtype, seed):
    B, H, W = size
    g = torch.Generator().manual_seed(seed)
    h = _cl(torch.randn(B, CMID, H, W, generator=g), dtype)
    x1, x2 = _cl(torch.randn(B, C1, H, W, generator=g), dtype), _cl(torch.randn(B, C2, H, W, generator=g), dtype)
    w = _cl(torch.randn(Cout, CMID, 3, 3, generator=g) / (3 * CMID ** 0.5), dtype)
    wsc = (torch.randn(Cout, C1 + C2, 1, 1, generator=g) / (C1 + C2) ** 0.5).to(dtype).to(DEV)
    b, bsc = (torch.randn(Cout, generator=g) * 0.3).to(dtype).to(DEV), (torch.randn(Cout, generator=g) * 0.3).to(dtype).to(DEV)
    return h, w, b, x1, x2, wsc, bsc


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("size", SIZES, ids=_ids)
@pytest.mark.parametrize("parts", PARTS, ids=_ids)
def test_shortcut_slabs_equal_the_one_source_op_for_every_tile_and_split(parts, size, dtype):
    ops = _ops()
    C1, C2 = parts
    for Cout in (64, 128):
        h, w, b, x1, x2, wsc, bsc = _tail_inputs(size, C1, C2, Cout, dtype, seed=C1 + 3 * C2 + Cout)
        cat = torch.cat([x1, x2], dim=1).contiguous(memory_format=CL)
        for tile_n in [0] + [tn for co, tn in TILES if co == Cout]:
            for splitk in _splits(C1, C2):
                want = ops.conv3x3_shortcut(h, w, b, cat, wsc, bsc, tile_n=tile_n, splitk=splitk)
                got = ops.conv3x3_shortcut_cat(h, w, b, x1, x2, wsc, bsc, tile_n=tile_n, splitk=splitk)
                assert got.shape == want.shape and got.dtype == dtype and got.is_contiguous(memory_format=CL)
                bad = got != want
                assert not bad.any(), "parts %s Cout %d tile_n %d splitk %d: %d of %d differ, first at %s" % (
                    parts, Cout, tile_n, splitk, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
        assert want.float().abs().max() > 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_probe_each_part_through_a_one_hot_shortcut(dtype):
    """h = 0 and one nonzero pixel in ONE part, a one-hot shortcut weight on that channel of the concatenation: the output is nonzero at that
    pixel and channel only -- x1 is read with pitch C1, x2 with pitch C2 from channel c - C1, the weight row with pitch C1 + C2."""
    ops = _ops()
    B, H, W, C1, C2, Cout = 2, 8, 8, 64, 128, 128
    g = torch.Generator().manual_seed(5)
    w = _cl(torch.randn(Cout, CMID, 3, 3, generator=g), dtype)
    h = torch.zeros(B, CMID, H, W, dtype=dtype, device=DEV).contiguous(memory_format=CL)
    zero = torch.zeros(Cout, dtype=dtype, device=DEV)
    for (pb, py, px), c0, n0 in (((0, 0, 0), 0, 0), ((1, 7, 7), C1 + C2 - 1, Cout - 1), ((1, 0, 7), C1 - 1, 65), ((0, 7, 0), C1, 3), ((1, 3, 4), C1 + 64, 64)):
        parts = [torch.zeros(B, C1, H, W, dtype=dtype, device=DEV).contiguous(memory_format=CL), torch.zeros(B, C2, H, W, dtype=dtype, device=DEV).contiguous(memory_format=CL)]
        parts[c0 >= C1][pb, c0 - (C1 if c0 >= C1 else 0), py, px] = 3.0
        wsc = torch.zeros(Cout, C1 + C2, 1, 1, dtype=dtype, device=DEV)
        wsc[n0, c0] = 0.5
        want = torch.zeros(B, Cout, H, W, dtype=dtype)
        want[pb, n0, py, px] = 1.5
        for tile_n, splitk in ((64, 1), (128, 1), (128, 7), (64, 12)):
            y = ops.conv3x3_shortcut_cat(h, w, zero, parts[0], parts[1], wsc, zero, tile_n=tile_n, splitk=splitk).cpu()
            assert torch.equal(y, want), ((pb, py, px), c0, n0, tile_n, splitk, y.nonzero().tolist()[:8])


def test_shortcut_declines_what_the_kernel_does_not_take():
    ops = _ops()
    h, w, b, x1, x2, wsc, bsc = _tail_inputs((1, 5, 7), 64, 128, 64, torch.bfloat16, seed=1)
    assert ops.conv3x3_shortcut_cat_takes(h, w, x1, x2, wsc)
    assert not ops.conv3x3_shortcut_cat_takes(h, w, x1.contiguous(), x2, wsc)                        # NCHW part
    assert not ops.conv3x3_shortcut_cat_takes(h, w, x1, x2[:, :, :4], wsc)                           # another size
    assert not ops.conv3x3_shortcut_cat_takes(h, w, x1.half(), x2.half(), wsc.half())                # another dtype than h
    assert not ops.conv3x3_shortcut_cat_takes(h, w, x1[:, :32].contiguous(memory_format=CL), x2, wsc[:, :160].contiguous())      # C1 = 32: off the 64 grid
    assert not ops.conv3x3_shortcut_cat_takes(h, w, x1, x2, wsc[:, :128].contiguous())               # a weight over fewer channels
    with pytest.raises(ops.PwwHipError, match="exceeds the 12 K-slabs"):
        ops.conv3x3_shortcut_cat(h, w, b, x1, x2, wsc, bsc, splitk=13)
    with pytest.raises(ops.PwwHipError, match="shortcut_bias"):
        ops.conv3x3_shortcut_cat(h, w, b, x1, x2, wsc, bsc[:32])


# ---- the restated up block ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("has_attn", [False, True], ids=["plain", "attn"])
def test_up_block_with_the_switch_on_and_off(has_attn, dtype, monkeypatch):
    """One stand-in UpBlock (prev 64, skips 64 / 128, out 64, 8 x 8): PWW_CONCAT 1 and 0 give the same bits, the counter says which way each
    of the two resnets went, and NCHW inputs decline to the stock sequence with the same result as the switch off."""
    import pww_hip.blocks as blocks
    from sd_standin import unet as U
    torch.manual_seed(0)
    block = U.UpBlock(128, 64, 64, 64, 2, 2, 96, has_attn, False, 32, False).to(dtype).eval().requires_grad_(False).to(DEV).to(memory_format=CL)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 8, 8, generator=g).to(dtype).to(DEV)
    skips = (torch.randn(2, 128, 8, 8, generator=g).to(dtype).to(DEV), torch.randn(2, 64, 8, 8, generator=g).to(dtype).to(DEV))
    temb, ctx = torch.randn(2, 64, generator=g).to(dtype).to(DEV), torch.randn(2, 5, 96, generator=g).to(dtype).to(DEV)
    xc, sc = x.contiguous(memory_format=CL), tuple(s.contiguous(memory_format=CL) for s in skips)
    out = {}
    with torch.no_grad():
        blocks.install_blocks(block)
        try:
            for on in (True, False):
                monkeypatch.setattr(blocks, "CONCAT", on)
                blocks.reset_stats()
                out[on], left = block(xc, sc, temb, ctx)
                st = blocks.stats()
                assert left == () and st["concat"] == ({"fused": 2, "declined": 0} if on else {"fused": 0, "declined": 0}), st
                assert st["conv_shortcut"] == {"fused": 2, "declined": 0} and st["resnet_block"] == {"fused": 2, "declined": 0} and st["group_norm"]["declined"] == 0, st
                assert st["conv3x3"]["declined"] == 0 and st["conv3x3"]["fused"] == 4, st
            assert torch.equal(out[True], out[False]) and out[True].is_contiguous(memory_format=CL)
            # NCHW inputs: both resnets decline, the concatenation is made, and the result is that of the switch off on the same inputs
            # (NCHW tensors reach MIOpen's convolutions: its deterministic solvers only, and the switch off before AND after, so that the
            # stock sequence is seen to repeat itself before anything is held to it)
            runs, deterministic = [], torch.backends.cudnn.deterministic
            torch.backends.cudnn.deterministic = True
            try:
                for on in (False, False, True, False):
                    monkeypatch.setattr(blocks, "CONCAT", on)
                    blocks.reset_stats()
                    runs.append(block(x, skips, temb, ctx)[0])
                    assert blocks.stats()["concat"] == ({"fused": 0, "declined": 2} if on else {"fused": 0, "declined": 0})
            finally:
                torch.backends.cudnn.deterministic = deterministic
            print("NCHW decline %s: stock run 2 == run 4: %s, declined == run 2: %s, max |diff| %.3e" % (
                dtype, torch.equal(runs[1], runs[3]), torch.equal(runs[2], runs[1]), (runs[2].float() - runs[1].float()).abs().max().item()))
            assert torch.equal(runs[2], runs[1]) and torch.equal(runs[2], runs[3])
        finally:
            blocks.uninstall_blocks(block)
        assert "forward" not in block.__dict__
        assert torch.isfinite(out[True].float()).all() and out[True].float().abs().max() > 0.1
