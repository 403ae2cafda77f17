"""Shapes, seeded inputs and the reference of the norm kernels' tests (csrc/pww_norm.hip, csrc/pww_blocks.hip), shared by the GPU tests
(test_norm_gpu.py: the SD shapes; test_norm_edges_gpu.py: every launch form, pre_bias, other group counts, float16 statistics) and the
host test that holds the reference to the stock CPU sequence and the table's launch forms to the library's own plan
(test_norm_cases_host.py). Test infrastructure."""
import torch
import torch.nn.functional as F

ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
DTYPES = [torch.bfloat16, torch.float16]


def reference(x, add, weight, bias, groups, eps, act, dtype, pre=None):
    """fp32 / fp64 torch with the kernel's rounding points (NCHW logical layout): h = T(x + pre), then T(h + add); statistics of the
    T-rounded h in fp64; the normalised value rounded to T before the activation."""
    h = x.float()
    if pre is not None:
        h = (h + pre.float()[None, :, None, None]).to(dtype).float()
    if add is not None:
        h = (h + add.float()[:, :, None, None]).to(dtype).float()
    B, C, H, W = h.shape
    hd = h.double().reshape(B, groups, -1)
    mean = hd.mean(-1)
    var = hd.var(-1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    a = rstd[:, :, None] * (weight.float() if weight is not None else torch.ones(C, device=x.device)).reshape(1, groups, -1)
    b = (bias.float() if bias is not None else torch.zeros(C, device=x.device)).reshape(1, groups, -1) - a * mean.float()[:, :, None]
    y = (h * a.reshape(B, C, 1, 1) + b.reshape(B, C, 1, 1)).to(dtype).float()
    if act == "silu":
        y = y / (1.0 + torch.exp(-y))
    return y.to(dtype)


def stock(x, add, weight, bias, groups, eps, act, pre=None, norm_in_fp32=False):
    """The op sequence the fused kernel replaces, on tensors of x's type: the adds, F.group_norm, F.silu. norm_in_fp32: the norm and the
    activation on fp32 copies, rounded after each (what the half-precision operators compute, for a CPU without them)."""
    h = x
    if pre is not None:
        h = h + pre[None, :, None, None]
    if add is not None:
        h = h + add[:, :, None, None]
    if not norm_in_fp32:
        y = F.group_norm(h, groups, weight, bias, eps)
        return F.silu(y) if act == "silu" else y
    y = F.group_norm(h.float(), groups, None if weight is None else weight.float(), None if bias is None else bias.float(), eps).to(x.dtype)
    return F.silu(y.float()).to(x.dtype) if act == "silu" else y


def close(y, ref, dtype, steps=1):
    """(elements further than `steps` rounding steps of dtype from ref, max |y - ref| / max |ref|); a step is relative to the element,
    with a floor of 1e-2 of the tensor's maximum."""
    yf, rf = y.float(), ref.float()
    tol = steps * ULP[dtype] * (rf.abs() + 1e-2 * rf.abs().max())
    bad = ((yf - rf).abs() > tol)
    return int(bad.sum()), float((yf - rf).abs().max() / rf.abs().max())


# ---- GroupNorm: (B, C, H, W, G) -> the launch form per layout ----------------------------------------------------------------------------
# "group": one launch, workgroup = (group, image) (gn_group_*); ("two", nslab): gn_moments_* + gn_apply_* with nslab partials per (image,
# group); None: the row is not there for that layout's form (it still runs). NHWC on more than 2048 channels runs the two-launch form on
# 512 threads. PLs = 256 / (cg / 4) is the single-launch NHWC form's pixels in flight, cg = C / G.
GN_CASES = [
    # NHWC 512 threads, 320 busy, 9-pixel slabs (a masked second trip) | NCHW TPR 72 / RP 3, 12 rows per workgroup over 5120 rows (row tail)
    ((2, 2560, 24, 24, 32), ("two", 64), ("two", 2)),
    ((2, 2240, 8, 37, 28), ("two", 37), ("two", 1)),            # 512 threads, 280 busy, G = 28 | TPR 37
    ((3, 2056, 8, 10, 8), ("two", 10), "group"),                # the smallest C on the 512 form (257 busy), cg = 257
    ((2, 4096, 5, 8, 32), "group", "group"),                    # single launch at the largest C
    ((1, 320, 24, 25, 8), "group", ("two", 1)),                 # PLs = 25: exactly 24 full pieces
    ((1, 320, 8, 74, 8), "group", ("two", 1)),                  # 24 pieces, the last ragged (592 = 23 * 25 + 17)
    ((1, 320, 19, 32, 8), ("two", 13), ("two", 1)),             # 25 pieces
    ((1, 1024, 4, 6, 1), "group", ("two", 1)),                  # G = 1, cg = 1024, one pixel in flight, 24 pieces | TPR 3 / RP 85
    ((2, 16, 104, 104, 1), ("two", 11), ("two", 10)),           # G = 1; 11 slabs, the last 576 of 1024 pixels | 6 chunks per thread and row
    ((2, 8, 8, 1, 1), "group", "group"),                        # the smallest legal tensor; HW < PLs
    ((2, 48, 6, 4, 3), "group", "group"),                       # HW < PLs; G = 3
    ((2, 96, 5, 8, 24), "group", "group"),                      # HW < PLs; G = 24
    ((3, 40, 8, 9, 5), "group", "group"),                       # HW < PLs; G = 5
    ((2, 48, 4, 6, 8), ("two", 1), None),                       # cg = 6: no 4-channel pieces, 8-channel chunks straddle groups
    ((1, 16, 48, 64, 8), None, "group"),                        # NCHW kper 2 with a chunk tail (384 chunks per row on 256 threads)
    ((2, 64, 64, 128, 32), None, "group"),                      # NCHW kper 4
    ((1, 96, 32, 64, 8), None, "group"),                        # NCHW exactly 12 pieces
    ((1, 104, 32, 64, 8), None, ("two", 1)),                    # NCHW 13 pieces
    # NHWC 512 busy on the 512 form, ONE partial: the workspace query answers 16 bytes like the single-launch form | one thread per row
    ((1, 4096, 2, 4, 1), None, ("two", 2)),
]
GN_SHAPES = [c[0] for c in GN_CASES]
ADDENDS = [(False, False), (True, False), (False, True), (True, True)]          # (pre, add)
ACTS = [None, "silu"]
# one shape per kernel for weight only / bias only / neither: (shape, channels_last) -- gn_group_nhwc, gn_group_nchw, gn_moments_nhwc +
# gn_apply_nhwc on 256 and on 512 threads, gn_moments_nchw + gn_apply_nchw
AFFINE_CASES = [((2, 96, 5, 8, 24), True), ((2, 96, 5, 8, 24), False), ((1, 320, 19, 32, 8), True), ((3, 2056, 8, 10, 8), True),
                ((1, 320, 19, 32, 8), False)]
AFFINE = [(True, False), (False, True), (False, False)]                         # (weight, bias)
IN_PLACE = (1, 320, 19, 32, 8)                                                  # two-launch in both layouts


def gn_inputs(shape, dtype):
    """(x, weight, bias, add, pre) on the CPU in `dtype`, seeded by the shape: the recipe of test_group_norm_matches_the_fp32_reference
    (per-channel offsets of 0.4 under a spread of 1.7) + pre = 0.5 * randn(C)."""
    B, C, H, W = shape[:4]
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + C + H)
    x = (torch.randn((B, C, H, W), generator=g) * 1.7 + 0.4 * torch.randn(1, C, 1, 1, generator=g)).to(dtype)
    w = (1.0 + 0.3 * torch.randn(C, generator=g)).to(dtype)
    b = (0.2 * torch.randn(C, generator=g)).to(dtype)
    add = (0.8 * torch.randn(B, C, generator=g)).to(dtype)
    pre = (0.5 * torch.randn(C, generator=g)).to(dtype)
    return x, w, b, add, pre


# ---- float16 statistics under a large mean: one shape per accumulating kernel, (mean, sigma) ---------------------------------------------
STAT_SHAPES = [(2, 640, 32, 32, 32),        # single launch in both layouts
               (2, 320, 64, 64, 32),        # two launches in both
               (2, 2560, 24, 24, 32),       # NHWC on 512 threads
               (2, 64, 64, 128, 32)]        # NCHW single launch with kper 4
STAT_REGIMES = [(300.0, 0.5), (30.0, 0.5), (60.0, 1.0)]


def stat_noise(shape):
    """fp32 standard normal [B, C, H, W] on the CPU, seeded by the shape."""
    B, C, H, W = shape[:4]
    return torch.randn((B, C, H, W), generator=torch.Generator(device="cpu").manual_seed(5 + C + H))


# ---- add + LayerNorm --------------------------------------------------------------------------------------------------------------------
# C around the boundaries of the kernel's chunks-per-lane template (512 / 1024 / 1536 channels), the smallest and the largest
LN_CHANNELS = [8, 504, 512, 520, 1024, 1032, 1536, 1544, 2040, 2048]
LN_ROWS = [1, 5]
LN_REFUSED = [2056, 12]


def ln_inputs(rows, C, dtype):
    """(x, a, weight, bias, post_bias) on the CPU: the recipe of test_add_layer_norm_matches_the_stock_sequence + post_bias."""
    g = torch.Generator(device="cpu").manual_seed(rows + C)
    x = (torch.randn((rows, C), generator=g) * 2.0 + 0.3).to(dtype)
    a = torch.randn((rows, C), generator=g).to(dtype)
    w = (1.0 + 0.2 * torch.randn(C, generator=g)).to(dtype)
    b = (0.1 * torch.randn(C, generator=g)).to(dtype)
    pb = (0.5 * torch.randn(C, generator=g)).to(dtype)
    return x, a, w, b, pb
