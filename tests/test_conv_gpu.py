"""GPU tests of pww_conv3x3_fwd (csrc/pww_conv.hip: 3 x 3 convolution as an implicit GEMM over NHWC) and of its routes in pww_hip/blocks.py.

Reference = fp32 F.conv2d of the same (rounded) inputs. Bar: one rounding step of the storage type relative to the output's spread,
|y - ref| <= 2 ULP (s + 1e-2 max s), s = |ref| (+ |conv| with a bias: the conv is rounded before the bias is added) -- fp32 accumulation, one rounding. The epilogue (bias, bias + residual) must reproduce
the stock sequence's rounding points exactly: bitwise equal to the kernel's own no-epilogue result followed by pww_bias_residual.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
CL = torch.channels_last
# (Cin, Cout, output size, stride, upsample) of the SD1.5 UNet's 3 x 3 convolutions (tools/time_conv3x3.py: with their counts)
SHAPES = [(320, 320, 64, 1, 0), (640, 640, 64, 1, 1), (960, 320, 64, 1, 0), (640, 320, 64, 1, 0),
          (320, 320, 32, 2, 0), (320, 640, 32, 1, 0), (640, 640, 32, 1, 0), (1280, 1280, 32, 1, 1), (1920, 640, 32, 1, 0),
          (1280, 640, 32, 1, 0), (960, 640, 32, 1, 0),
          (640, 640, 16, 2, 0), (640, 1280, 16, 1, 0), (1280, 1280, 16, 1, 0), (1280, 1280, 16, 1, 1), (2560, 1280, 16, 1, 0), (1920, 1280, 16, 1, 0),
          (1280, 1280, 8, 2, 0), (1280, 1280, 8, 1, 0), (2560, 1280, 8, 1, 0)]


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
    """fp32 conv (+ bias) of the rounded inputs, and the magnitude the bar scales with: with a bias the kernel rounds the conv before adding
    it (the stock rounding points), so a rounding step of |conv| -- not only of |conv + bias| -- is within the bar."""
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


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d-s%d-u%d" % s)
def test_unet_shapes_two_rows_bf16(shape):
    Cin, Cout, S, stride, up = shape
    Hin = S * stride // (2 if up else 1)
    x, w, b = _inputs(2, Cin, Cout, Hin, Hin, torch.bfloat16)
    y = _ops().conv3x3(x, w, b if up else None, stride=stride, upsample=bool(up))
    _check(y, _reference(x, w, b if up else None, stride, up), torch.bfloat16)


@pytest.mark.parametrize("shape", [SHAPES[i] for i in (0, 1, 4, 7, 12, 15, 18)], ids=lambda s: "%d-%d-%d-s%d-u%d" % s)
def test_unet_shapes_sixteen_rows(shape):
    Cin, Cout, S, stride, up = shape
    Hin = S * stride // (2 if up else 1)
    x, w, b = _inputs(16, Cin, Cout, Hin, Hin, torch.bfloat16, seed=1)
    y = _ops().conv3x3(x, w, b, stride=stride, upsample=bool(up))
    _check(y, _reference(x, w, b, stride, up), torch.bfloat16)


@pytest.mark.parametrize("shape", [SHAPES[i] for i in (0, 1, 4, 8, 13, 17, 19)], ids=lambda s: "%d-%d-%d-s%d-u%d" % s)
def test_fp16(shape):
    Cin, Cout, S, stride, up = shape
    Hin = S * stride // (2 if up else 1)
    x, w, b = _inputs(2, Cin, Cout, Hin, Hin, torch.float16, seed=2)
    y = _ops().conv3x3(x, w, b, stride=stride, upsample=bool(up))
    _check(y, _reference(x, w, b, stride, up), torch.float16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tile_n,splitk", [(64, 1), (128, 1), (128, 5), (64, 7)])
def test_epilogue_rounding_points_exact(dtype, tile_n, splitk):
    """bias: T(T(conv) + b); bias + residual: T(r + T(T(conv) + b)) -- bitwise what conv -> pww_bias_residual gives."""
    ops = _ops()
    x, w, b = _inputs(2, 640, 1280, 16, 16, dtype, seed=3)
    r = torch.randn(2, 1280, 16, 16, device=DEV).to(dtype).contiguous(memory_format=CL)
    plain = ops.conv3x3(x, w, tile_n=tile_n, splitk=splitk)
    with_bias = ops.conv3x3(x, w, b, tile_n=tile_n, splitk=splitk)
    assert torch.equal(with_bias, (plain.float() + b.float()[None, :, None, None]).to(dtype))
    fused = ops.conv3x3(x, w, b, residual=r, tile_n=tile_n, splitk=splitk)
    assert torch.equal(fused, ops.bias_residual(r, plain, b))
    _check(plain, _reference(x, w, None, 1, 0), dtype)


@pytest.mark.parametrize("splitk", [0, 1, 3, 8])
def test_bitwise_repeatable_and_graph_replay(splitk):
    ops = _ops()
    x, w, b = _inputs(2, 1280, 1280, 8, 8, torch.bfloat16, seed=4)
    r = torch.randn(2, 1280, 8, 8, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
    eager = [ops.conv3x3(x, w, b, residual=r, splitk=splitk) for _ in range(3)]
    assert all(torch.equal(eager[0], e) for e in eager[1:])
    out = {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.conv3x3(x, w, b, residual=r, splitk=splitk)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out["y"] = ops.conv3x3(x, w, b, residual=r, splitk=splitk)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["y"], eager[0])


@pytest.mark.parametrize("Cin,H,W,stride,up", [(64, 8, 8, 1, 0), (128, 5, 7, 1, 0), (64, 9, 11, 2, 0), (128, 3, 5, 1, 1), (64, 33, 17, 1, 0)])
def test_small_and_ragged_widths(Cin, H, W, stride, up):
    """tiny-config widths, odd spatial sizes (the M tail of a 128-row tile, halo on every side) and odd strided / upsampled sizes."""
    ops = _ops()
    x, w, b = _inputs(3, Cin, 128, H, W, torch.bfloat16, seed=5)
    assert ops.conv3x3_takes(x, w, stride, bool(up))
    y = ops.conv3x3(x, w, b, stride=stride, upsample=bool(up))
    _check(y, _reference(x, w, b, stride, up), torch.bfloat16)


# (Cin, splitk): the slabs per split, n = s_end - s_begin with s = ks * nslab / splitk. Cin 64 has 9 K-slabs, one per tap; Cin 128 has 18, two
# per tap, so that an odd s_begin starts in the middle of a tap (ci0 = 64).
SHORT_SPLITS = [(64, 3), (64, 4), (64, 5), (64, 9),         # n = 3;  2 or 3;  1 or 2;  1
                (128, 5), (128, 7), (128, 9), (128, 18)]    # n = 3 or 4;  2 or 3;  2;  1
SHORT_GEOMETRIES = [(3, 5, 7, 1, 0), (2, 9, 11, 2, 0), (2, 3, 5, 1, 1)]     # (rows, Hin, Win, stride, upsample): M = 105, 60, 120 -- a lone partial tile
_SHORT_CASES = {}


def _short_case(Cin, geometry, dtype):
    """Inputs, residual and the two fp32 references (plain, with bias) of one short-split case, computed once and left unchanged."""
    key = (Cin, geometry, dtype)
    if key not in _SHORT_CASES:
        rows, Hin, Win, stride, up = geometry
        x, w, b = _inputs(rows, Cin, 128, Hin, Win, dtype, seed=6)
        plain_ref, bias_ref = _reference(x, w, None, stride, up), _reference(x, w, b, stride, up)
        r = torch.randn(plain_ref[0].shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7)).to(dtype).contiguous(memory_format=CL)
        _SHORT_CASES[key] = (x, w, b, r, plain_ref, bias_ref)
    return _SHORT_CASES[key]


def _ulp_ratio(y, ref_scale, dtype):
    """max |y - ref| in units of the bar's one-step term ULP (s + 1e-2 max s): _check passes up to 2."""
    ref, scale = ref_scale
    return ((y.float() - ref).abs() / (ULP[dtype] * (scale + 1e-2 * scale.max()))).max().item()


def test_short_split_counts():
    """The splits above really give the slab counts they are there for, by the kernel's own s_begin / s_end arithmetic."""
    want = {(64, 3): ({3}, False), (64, 4): ({2, 3}, False), (64, 5): ({1, 2}, False), (64, 9): ({1}, False),
            (128, 5): ({3, 4}, True), (128, 7): ({2, 3}, True), (128, 9): ({2}, False), (128, 18): ({1}, True)}
    for Cin, ns in SHORT_SPLITS:
        nslab, per_tap = 9 * Cin // 64, Cin // 64
        begins = [ks * nslab // ns for ks in range(ns + 1)]
        counts = {b - a for a, b in zip(begins, begins[1:])}
        mid_tap = any(s % per_tap for s in begins[:-1])
        assert (counts, mid_tap) == want[(Cin, ns)], (Cin, ns, counts, mid_tap)
        assert max(counts) <= 4 and min(counts) < 4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tile_n", [64, 128])
@pytest.mark.parametrize("geometry", SHORT_GEOMETRIES, ids=lambda g: "%dx%dx%d-s%d-u%d" % g)
@pytest.mark.parametrize("Cin,splitk", SHORT_SPLITS)
def test_short_splits(Cin, splitk, geometry, tile_n, dtype):
    """Splits of 1, 2 and 3 K-slabs: the K loop's steady part needs 4, so these run in the drain alone -- its conditional requests and moves,
    with a split that starts in the middle of a tap at Cin 128. The planner never picks such a split (at least 8 slabs each), but `splitk` is a
    public field. Plain, with bias, with bias + residual: the 2-ULP bar, the exact-epilogue identities, three bitwise equal calls.
    (A drain that moved register set t % PF instead of (t + 1) % PF would compute slab 0 twice in every n >= 2 split; a ci0 that started at 0
    would read the wrong 64 channels in the Cin 128 splits that begin at an odd slab. Both land far outside the bar.)"""
    ops = _ops()
    rows, Hin, Win, stride, up = geometry
    x, w, b, r, plain_ref, bias_ref = _short_case(Cin, geometry, dtype)
    kw = dict(stride=stride, upsample=bool(up), tile_n=tile_n, splitk=splitk)
    plain = ops.conv3x3(x, w, **kw)
    with_bias = ops.conv3x3(x, w, b, **kw)
    fused = [ops.conv3x3(x, w, b, residual=r, **kw) for _ in range(3)]
    print("short split Cin %d splitk %d %s tile_n %d %s: |err| / (ULP (s + 1e-2 max s)) plain %.3f, bias %.3f (bar 2)"
          % (Cin, splitk, geometry, tile_n, dtype, _ulp_ratio(plain, plain_ref, dtype), _ulp_ratio(with_bias, bias_ref, dtype)))
    _check(plain, plain_ref, dtype)
    _check(with_bias, bias_ref, dtype)
    assert torch.equal(with_bias, (plain.float() + b.float()[None, :, None, None]).to(dtype))
    assert torch.equal(fused[0], ops.bias_residual(r, plain, b))
    assert torch.equal(fused[0], fused[1]) and torch.equal(fused[0], fused[2])
    assert torch.equal(plain, ops.conv3x3(x, w, **kw)) and torch.equal(with_bias, ops.conv3x3(x, w, b, **kw))


def test_more_splits_than_slabs_is_refused():
    ops = _ops()
    x, w, _ = _inputs(3, 64, 128, 5, 7, torch.bfloat16, seed=6)
    with pytest.raises(ops.PwwHipError, match="exceeds the 9 K-slabs"):
        ops.conv3x3(x, w, splitk=10)
    assert ops.conv3x3(x, w, splitk=9).shape == (3, 128, 5, 7)


def test_declines():
    ops = _ops()
    x, w, _ = _inputs(2, 64, 64, 8, 8, torch.bfloat16)
    assert not ops.conv3x3_takes(x.contiguous(), w)                                   # NCHW keeps MIOpen
    assert not ops.conv3x3_takes(x.float(), w.float())                                # fp32
    assert not ops.conv3x3_takes(x[:, :32].contiguous(memory_format=CL), w[:, :32])    # Cin 32: no tile
    x4, w4, _ = _inputs(2, 4, 320, 8, 8, torch.bfloat16)
    assert not ops.conv3x3_takes(x4, w4)                                               # conv_in
    assert not ops.conv3x3_takes(x, w[:4])                                             # conv_out (Cout 4)
    assert not ops.conv3x3_takes(x, w, stride=3)
    with pytest.raises(Exception):
        ops.conv3x3(x.contiguous(), w)


def test_blocks_route_resnet_down_up_and_plain_convs():
    """The stand-in UNet's ResnetBlock2D (conv1, conv2 + bias + residual), Downsample2D, Upsample2D and a plain 3 x 3 conv through
    install_blocks against the module's own forward: same result within the bar, the conv3x3 counter moves, NCHW declines."""
    import pww_hip.blocks as blocks
    from sd_standin import unet as U
    torch.manual_seed(0)
    res = U.ResnetBlock2D(128, 192, 256, 32).to(DEV, torch.bfloat16).eval()
    down = U.Downsample2D(192).to(DEV, torch.bfloat16).eval()
    up = U.Upsample2D(192).to(DEV, torch.bfloat16).eval()
    plain = nn.Sequential(nn.Conv2d(192, 128, 3, padding=1)).to(DEV, torch.bfloat16).eval()
    mods = nn.ModuleList([res, down, up, plain]).to(memory_format=CL)
    x = torch.randn(2, 128, 16, 16, device=DEV).to(torch.bfloat16).contiguous(memory_format=CL)
    temb = torch.randn(2, 256, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        ref_h = res(x, temb)
        ref = [ref_h, down(ref_h), up(ref_h), plain(ref_h)]
        blocks.install_blocks(mods)
        try:
            blocks.reset_stats()
            h = res(x, temb)
            got = [h, down(ref_h), up(ref_h), plain(ref_h)]
            st = blocks.stats()
            assert st["conv3x3"]["fused"] == 5 and st["conv3x3"]["declined"] == 0, st
            assert st["hit_rate"] == 1.0
            for g_, r_ in zip(got, ref):
                assert g_.shape == r_.shape
                err = (g_.float() - r_.float()).abs().max().item()
                assert err <= 16 * ULP[torch.bfloat16] * r_.float().abs().max().item(), err
            blocks.reset_stats()
            y = plain(ref_h.contiguous())                          # NCHW: the module's own forward
            assert blocks.stats()["conv3x3"]["declined"] == 1 and y.shape == ref[3].shape
        finally:
            blocks.uninstall_blocks(mods)
