"""Edge shapes of the request-preparation kernels (csrc/pww_mask.hip) through pww_hip.ops, against the oracle and plain numpy / fp64.

The product reaches these kernels on its own images only (512 x 512, 768 x 768, 384 x 448, 500 x 500; 3 - 5 regions; T = 77). Here:
one-pixel levels, levels under one workgroup and one pixel over it, 64 regions, column lists that name every region / a region twice /
nothing, other prompt lengths, a grid-stride loop that runs more than once, ragged ends, the smallest legal blur, non-integer nearest
scales. Inputs are seeded and synthetic (tests/prep_cases.py); tests/test_oracle_shapes_host.py holds the oracle to torch at the same
shapes. "Bit for bit" compares the int32 views, so a flipped sign of zero or another NaN counts.

One-line changes of each kernel that a case here turns into a failure, argued from the code:
  mask_build_kernel<RgbTap / F32Tap>  level lookup `blockIdx.x > blk0[i]` for `>=`: at 32 x 32 the levels' first workgroups are 0, 1, 2, 3, so block 1 takes
                        itself for level 0 at pix0 = 64, writes nothing, and the 4-pixel map stays unwritten. Column sum walked backwards:
                        test_mask_build_f32_sums_overlapping_regions_in_list_order. `lp = i / 77`: every T = 1 / T = 231 case.
                        `nlocal = MASK_PIX`: test_mask_build_writes_its_levels_and_nothing_after_them finds zeros in the guard after a 16-pixel level.
  resize_tokens_kernel  the 1-D nearest scale dropped (src = n): (16, 16, 3, 200), where oh * ow = 196 != 200. `ox = src % oh`: (20, 12, 5, 60).
  blur_rows / blur_cols `2 * (n - 1) - i` -> `2 * n - 1 - i` (or `-i` -> `-i - 1`): test_gauss_blur_single_pixel at (19, 19) / (0, 0).
  inpaint_prep_kernel   threshold on the byte moved by one (`>= 0.5f` against 127 / 255 or 128 / 255 flipped): the sampled pixels of every case hold 127 / 128.
                        sx from the row scale H / h: only where the two scales differ -- (33, 35, 4, 4): 8.25 for 8.75, x = 2 reads column 16 for 17 and
                        x = 3 reads 24 for 26; (48, 40, 4, 8): 12 for 5, x = 1 .. 7 read 12, 24, 36, 39, 39, 39, 39 for 5 .. 35. Those columns hold random
                        bytes, not the checkerboard (test_oracle_shapes_host.py asserts that the latent mask changes). The other cases have equal scales.
  cfg_combine_kernel<f16 / bf16>  the stride loop replaced by one `if (i < n)`: n = 2048 * 256 + 1 and 600 001 leave the words past 524 288 unwritten.
  store_f32_kernel      `threadIdx.x <= a.n`: word n loses the sentinel at n = 1 and n = 5."""
import numpy as np
import pytest
import torch

import prep_cases as P
from gpu_util import _blur_exact
from oracle import pww_oracle as O

pytestmark = pytest.mark.gpu


def _ops():
    from pww_hip import ops
    return ops


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(got, want):
    got, want = _bits(got), _bits(want)
    return got.shape == want.shape and np.array_equal(got, want)


# ---- mask_build ---------------------------------------------------------------------------------------------------------------------

BACKGROUND = (9, 9, 9)            # a map colour that is no region

# (R, prompt kind, T, cell)
MASK_PROMPTS = [(1, "mixed", 1, 5), (1, "mixed", 77, 3), (64, "all", 1, 3), (64, "all", 77, 3), (64, "mixed", 77, 3), (64, "mixed", 231, 3),
                (5, "mixed", 231, 5), (5, "none", 77, 5)]
_MASK_INPUTS = {}


def _mask_inputs(H, W, R, cell):
    """(rgb, colours, strengths, fp32 masks [R, H, W]) of one seeded map, built once."""
    key = (H, W, R, cell)
    if key not in _MASK_INPUTS:
        colours = P.palette(R)
        rgb = P.colour_map(H, W, colours + [BACKGROUND], seed=17 * H + W + R, cell=cell)
        s = P.strengths(R)
        _MASK_INPUTS[key] = (rgb, colours, s, P.region_masks(rgb, colours, s))
    return _MASK_INPUTS[key]


def _build_both(dev, rgb, colours, strength, masks, cols, ratios):
    ops = _ops()
    table = [c + (s,) for c, s in zip(colours, strength)]
    got_rgb = ops.mask_build(torch.from_numpy(rgb).to(dev), table, cols, ratios)
    got_f32 = ops.mask_build_f32(torch.from_numpy(masks).to(dev), cols, ratios)
    return {r: got_rgb[r].cpu().numpy() for r in ratios}, {r: got_f32[r].cpu().numpy() for r in ratios}


def _check_maps(dev, H, W, R, kind, T, cell, ratios):
    rgb, colours, strength, masks = _mask_inputs(H, W, R, cell)
    ids, tok = P.prompt(kind, R, T)
    regions = [(i, m) for i, m in zip(ids, masks)]
    cols = O.column_region_lists(regions, tok)
    got_rgb, got_f32 = _build_both(dev, rgb, colours, strength, masks, cols, ratios)
    for r in ratios:
        want = O.tokens_img_attention_weight(regions, tok, r)
        Hr, Wr = P.level_size(H, W, r)
        assert want.shape == (Hr * Wr, T)
        assert _same_bits(got_rgb[r], want), ("rgb", r, np.abs(got_rgb[r] - want).max())
        assert _same_bits(got_f32[r], want), ("f32", r, np.abs(got_f32[r] - want).max())
        assert _same_bits(got_rgb[r], got_f32[r])
        if kind == "none":
            assert not want.any()
    return got_rgb, regions, tok


@pytest.mark.parametrize("R,kind,T,cell", MASK_PROMPTS, ids=lambda v: str(v))
@pytest.mark.parametrize("H,W", P.MASK_SHAPES)
def test_mask_build_edge_shapes(gpu_device, H, W, R, kind, T, cell):
    """The four default ratios in ONE launch (pww_mask_build / pww_mask_build_f32_levels), both taps, bit for bit against the oracle:
    levels of one pixel, levels under a workgroup followed at once by the next level's first workgroup, 65 pixels, up to 64 regions
    with strengths whose fp32 sum depends on the order, one position that collects all of them, a phrase twice, positions with none."""
    _check_maps(gpu_device, H, W, R, kind, T, cell, P.DEFAULT_RATIOS)


@pytest.mark.parametrize("H,W", [(32, 32), (100, 36)])
def test_mask_build_f32_sums_overlapping_regions_in_list_order(gpu_device, H, W):
    """Regions of a colour map are disjoint, so at most four of them meet in one bilinear footprint. Float masks may overlap: 64 dense
    random masks, all collected by one position, make every output element a 64-term fp32 sum whose bits depend on the order -- summing
    the regions backwards gives other bits -- and the kernel must give the oracle's."""
    masks = (np.random.default_rng(H).random((64, H, W), dtype=np.float32) * np.array(P.strengths(64), np.float32)[:, None, None]).astype(np.float32)
    ids, tok = P.prompt("all", 64, 77)
    regions = [(i, m) for i, m in zip(ids, masks)]
    cols = O.column_region_lists(regions, tok)
    got = _ops().mask_build_f32(torch.from_numpy(masks).to(gpu_device), cols, P.DEFAULT_RATIOS + (1,))
    for r in P.DEFAULT_RATIOS + (1,):
        want = O.tokens_img_attention_weight(regions, tok, r)
        assert _same_bits(got[r], want), (r, np.abs(got[r].cpu().numpy() - want).max())
        assert not _same_bits(O.tokens_img_attention_weight(regions[::-1], tok, r), want)


@pytest.mark.parametrize("H,W", [(32, 32), (100, 36)])
def test_mask_build_writes_its_levels_and_nothing_after_them(gpu_device, H, W):
    """The C entry points on ONE sentinel-filled slab: each level's output is a slice of it, followed by a guard of 64 * T floats -- what the
    last workgroup of a level would overrun if it took its 16, 4, 1 or 1 pixels for a full block of 64 (`nlocal = MASK_PIX`). With outputs
    that ops allocates one by one such an overrun lands in some neighbouring allocation and nobody looks. The levels hold the oracle's bits,
    the guards still hold the sentinel."""
    from pww_hip import _lib
    ops = _ops()
    dev, T, R, GUARD, FILL = gpu_device, 77, 5, 64 * 77, -777.25
    rgb, colours, strength, masks = _mask_inputs(H, W, R, 5)
    ids, tok = P.prompt("mixed", R, T)
    regions = [(i, m) for i, m in zip(ids, masks)]
    cols = O.column_region_lists(regions, tok)
    rows = [Hr * Wr for Hr, Wr in (P.level_size(H, W, r) for r in P.DEFAULT_RATIOS)]
    begin = [sum(rows[:i]) * T + i * GUARD for i in range(4)]
    total = begin[3] + rows[3] * T + GUARD
    rgb_d, masks_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(masks).to(dev)
    regs, (col_ptr, col_reg) = ops._regions_tensor([c + (s,) for c, s in zip(colours, strength)], dev), ops._csr(cols, dev)
    lib, p = _lib.load(), ops._ptr

    def run(call):
        slab = torch.full((total,), FILL, device=dev)
        outs = [slab[b:b + n * T] for b, n in zip(begin, rows)]
        with torch.cuda.device(dev):
            _lib.check(call(outs), "mask_build")
        return slab.cpu().numpy()

    slabs = [run(lambda o: lib.pww_mask_build(p(rgb_d), H, W, p(regs), R, p(col_ptr), p(col_reg), T, *[p(t) for t in o], ops._stream())),
             run(lambda o: lib.pww_mask_build_f32_levels(p(masks_d), H, W, R, p(col_ptr), p(col_reg), T, *[p(t) for t in o], ops._stream())),
             run(lambda o: lib.pww_mask_build_rgb(p(rgb_d), H, W, p(regs), R, p(col_ptr), p(col_reg), T, 8, p(o[0]), ops._stream())),
             run(lambda o: lib.pww_mask_build_f32(p(masks_d), H, W, R, p(col_ptr), p(col_reg), T, 16, p(o[1]), ops._stream()))]
    written = [(0, 1, 2, 3), (0, 1, 2, 3), (0,), (1,)]
    for slab, levels in zip(slabs, written):
        keep = np.ones(total, bool)
        for i in levels:
            want = O.tokens_img_attention_weight(regions, tok, P.DEFAULT_RATIOS[i])
            assert want.any() or rows[i] == 1
            assert _same_bits(slab[begin[i]:begin[i] + rows[i] * T].reshape(rows[i], T), want)
            keep[begin[i]:begin[i] + rows[i] * T] = False
        assert (slab[keep] == np.float32(FILL)).all(), int((slab[keep] != np.float32(FILL)).sum())


@pytest.mark.parametrize("ratios", P.RATIO_SETS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("R,kind,T,cell", [(64, "mixed", 77, 3), (5, "mixed", 231, 5)], ids=lambda v: str(v))
def test_mask_build_other_ratio_sets(gpu_device, ratios, R, kind, T, cell):
    """Ratio sets other than the default four go through the single-ratio entry points (pww_mask_build_rgb / pww_mask_build_f32) and,
    for the f32 tap with the four defaults among them, the mixed route. ratio 1 on the non-square map is the _ORIG map [H, W, T]."""
    H, W = P.RATIO_SHAPE
    got, regions, tok = _check_maps(gpu_device, H, W, R, kind, T, cell, ratios)
    if 1 in ratios:
        want = O.tokens_img_attention_weight(regions, tok, 1, original_shape=True)
        assert want.shape == (H, W, T) and _same_bits(got[1].reshape(H, W, T), want)


def test_mask_build_absent_colour_gives_zero_column(gpu_device):
    """A region whose colour the map does not hold contributes nothing: its own column is all zero, a shared column keeps the other
    region's values."""
    H, W = P.RATIO_SHAPE
    colours = P.palette(3) + [P.ABSENT]
    strength = P.strengths(4)
    rgb = P.colour_map(H, W, colours[:3], seed=5, cell=3)
    masks = P.region_masks(rgb, colours, strength)
    assert not masks[3].any()
    cols = [[], [0], [3], [], [1], [2, 3]]                     # position 2: the absent colour alone; position 5: region 2 and the absent one
    got_rgb, got_f32 = _build_both(gpu_device, rgb, colours, strength, masks, cols, P.DEFAULT_RATIOS + (1,))
    for r in P.DEFAULT_RATIOS + (1,):
        for got in (got_rgb[r], got_f32[r]):
            assert not got[:, 0].any() and not got[:, 2].any() and not got[:, 3].any()
            for col, region in ((1, 0), (4, 1), (5, 2)):
                assert _same_bits(got[:, col], O.bilinear_resize(masks[region], *P.level_size(H, W, r)).reshape(-1))
        assert got_rgb[8][:, 5].any()


def test_mask_build_refusals(gpu_device):
    """65 regions: PwwHipError, and nothing is written (the C entry point is called on sentinel-filled outputs). A 24 x 40 map has no
    pixel at ratio 64 (round(24 / 64) = 0): PwwHipError "too small for ratio", not a launch over an empty level."""
    from pww_hip import _lib
    ops = _ops()
    dev = gpu_device
    H, W, T = 32, 32, 77
    colours = P.palette(65)
    strength = P.strengths(65)
    rgb = torch.from_numpy(P.colour_map(H, W, colours, seed=1, cell=3)).to(dev)
    table = [c + (s,) for c, s in zip(colours, strength)]
    cols = [[r] if r < 65 else [] for r in range(T)]
    with pytest.raises(ops.PwwHipError):
        ops.mask_build(rgb, table, cols)
    with pytest.raises(ops.PwwHipError):
        ops.mask_build_f32(torch.zeros(65, H, W, device=dev), cols)
    SENTINEL = -777.25
    regs, (col_ptr, col_reg) = ops._regions_tensor(table, dev), ops._csr(cols, dev)
    outs = [torch.full((n, T), SENTINEL, device=dev) for n in (16, 4, 1, 1)]
    one = torch.full((16, T), SENTINEL, device=dev)
    masks = torch.zeros(65, H, W, device=dev)
    lib = _lib.load()
    p, s = ops._ptr, ops._stream()
    with torch.cuda.device(dev):
        calls = [lib.pww_mask_build(p(rgb), H, W, p(regs), 65, p(col_ptr), p(col_reg), T, *[p(o) for o in outs], s),
                 lib.pww_mask_build_f32_levels(p(masks), H, W, 65, p(col_ptr), p(col_reg), T, *[p(o) for o in outs], s),
                 lib.pww_mask_build_rgb(p(rgb), H, W, p(regs), 65, p(col_ptr), p(col_reg), T, 8, p(one), s),
                 lib.pww_mask_build_f32(p(masks), H, W, 65, p(col_ptr), p(col_reg), T, 8, p(one), s)]
    for rc in calls:
        with pytest.raises(ops.PwwHipError, match="region count 65"):
            _lib.check(rc, "mask_build")
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs + [one])
    # 64 regions on the same call are taken
    assert ops.mask_build(rgb, table[:64], [c if c != [64] else [] for c in cols])[8].shape == (16, T)
    small = torch.from_numpy(P.colour_map(24, 40, colours[:5], seed=2, cell=3)).to(dev)
    cols5 = [[r] if r < 5 else [] for r in range(T)]
    with pytest.raises(ops.PwwHipError, match="too small for ratio"):
        ops.mask_build(small, table[:5], cols5)
    with pytest.raises(ops.PwwHipError, match="too small for ratio"):
        ops.mask_build_f32(torch.zeros(5, 24, 40, device=dev), cols5)


# ---- resize_tokens ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,T,n", P.RESIZE_CASES)
def test_resize_tokens_edge_shapes(gpu_device, H, W, T, n):
    """The _ORIG fallback bit for bit against the oracle: oh * ow equal to, below and above n_tokens, oh == 1, ow == 1, T == 1, one token."""
    w = P.random_weights(H, W, T, seed=n)
    got = _ops().resize_tokens(torch.from_numpy(w).to(gpu_device), n)
    assert _same_bits(got, O.orig_weight_fallback(w, n))


def test_resize_tokens_refuses_more_tokens_than_pixels(gpu_device):
    ops = _ops()
    H, W, T, n = P.RESIZE_REFUSED
    with pytest.raises(ops.PwwHipError):
        ops.resize_tokens(torch.from_numpy(P.random_weights(H, W, T, seed=n)).to(gpu_device), n)


# ---- gauss_blur ---------------------------------------------------------------------------------------------------------------------

def _check_blur(dev, m, sigma, ksize, what):
    """<= 2e-7 against the fp64 convolution, <= 5e-6 against the oracle's fp32 conv2d: the bars of test_round2_gpu.py::test_gauss_blur_kernel
    for masks of magnitude 1.5."""
    got = _ops().gauss_blur(torch.from_numpy(m).to(dev), sigma, ksize).cpu().numpy()
    exact = _blur_exact(m, sigma, ksize)
    ref = O.gaussian_blur(m, sigma, ksize)
    e_exact, e_ref = np.abs(got - exact).max(), np.abs(got - ref).max()
    print(f"blur {what} {m.shape} ksize {ksize} sigma {sigma}: kernel vs fp64 {e_exact:.2e} (bar 2e-7), kernel vs oracle {e_ref:.2e} (bar 5e-6)")
    assert e_exact <= 2e-7 and e_ref <= 5e-6
    return got, exact


@pytest.mark.parametrize("sigma", P.BLUR_SIGMAS)
@pytest.mark.parametrize("H,W", P.BLUR_SIZES)
def test_gauss_blur_smallest_sizes(gpu_device, H, W, sigma):
    """Sides of 20 = ksize / 2 + 1 (the reflection reaches index 0 and index H - 1 from both sides) and 21, widths under and over 39."""
    _check_blur(gpu_device, P.blur_mask(H, W, seed=H + W), sigma, 39, "random")


@pytest.mark.parametrize("sigma", P.BLUR_SIGMAS)
def test_gauss_blur_other_ksize(gpu_device, sigma):
    (H, W), ks = P.BLUR_SMALL
    _check_blur(gpu_device, P.blur_mask(H, W, seed=4), sigma, ks, "random")


@pytest.mark.parametrize("y,x", [(0, 0), (0, 19), (19, 0), (19, 19), (10, 10)])
def test_gauss_blur_single_pixel(gpu_device, y, x):
    """One 1.5 pixel on 20 x 20: the result is the reflected kernel itself, 1.5 * a(y') a(x') with a(y') = the sum of the taps whose reflected
    index is the source row -- written out here from the padding rule, not taken from np.pad. A wrong reflection index misplaces the peak."""
    H = W = 20
    m = np.zeros((H, W), np.float32)
    m[y, x] = 1.5
    sigma = 4.0
    got, _ = _check_blur(gpu_device, m, sigma, 39, "delta (%d, %d)" % (y, x))
    k = _ops().gaussian_kernel1d(sigma, 39).double().numpy()

    def profile(src):
        a = np.zeros(H)
        for o in range(H):
            for j in range(39):
                i = o + j - 19
                i = -i if i < 0 else (2 * (H - 1) - i if i >= H else i)
                if i == src:
                    a[o] += k[j]
        return a
    want = 1.5 * np.outer(profile(y), profile(x))
    assert np.abs(got - want).max() <= 2e-7
    assert np.unravel_index(np.argmax(got), got.shape) == (y, x)


def test_gauss_blur_refusals(gpu_device):
    ops = _ops()
    with pytest.raises(ops.PwwHipError):
        ops.gauss_blur(torch.zeros(40, 40, device=gpu_device), 4.0, 38)          # even ksize
    with pytest.raises(ops.PwwHipError):
        ops.gauss_blur(torch.zeros(19, 40, device=gpu_device), 4.0, 39)          # ksize / 2 == H: the reflection would leave the image
    with pytest.raises(ops.PwwHipError):
        ops.gauss_blur(torch.zeros(40, 19, device=gpu_device), 4.0, 39)


# ---- inpaint_prep -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,h,w", P.INPAINT_CASES)
def test_inpaint_prep_edge_shapes(gpu_device, H, W, h, w):
    """Mask, masked image and latent-size mask bit for bit against the oracle: H * W no multiple of 256, non-square, H / h not an
    integer (500 -> 62: the fp32 floor(y * H / h) lands next to integers), h == H, a 1 x 1 latent; 127 / 128 on the sampled pixels."""
    from pww_hip import _lib
    ops = _ops()
    img, mask = P.inpaint_inputs(H, W, h, w, seed=7)
    rgb_d, mask_d = torch.from_numpy(img).to(gpu_device), torch.from_numpy(mask).to(gpu_device)
    m, masked, ml = ops.inpaint_prep(rgb_d, mask_d, h, w)
    om, omi = O.prepare_mask_and_masked_image(img, mask)
    assert m.shape == (1, 1, H, W) and masked.shape == (1, 3, H, W) and ml.shape == (1, 1, h, w)
    assert _same_bits(m, om.numpy()) and _same_bits(masked, omi.numpy())
    want_lat = O.nearest_resize(om.numpy(), h, w)
    assert _same_bits(ml, want_lat)
    if (H, W) != (h, w):                 # the sampled pixels hold 127 / 128 as a checkerboard over the latent grid: so does the latent mask
        assert np.array_equal(want_lat[0, 0], (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(np.float32))
    # without a latent mask (mask_lat == NULL) the pixel branch is the same, and h / w are not looked at
    m2, masked2 = torch.full_like(m, -3.0), torch.full_like(masked, -3.0)
    with torch.cuda.device(gpu_device):
        rc = _lib.load().pww_inpaint_prep(ops._ptr(rgb_d), ops._ptr(mask_d), H, W, 0, 0, ops._ptr(m2), ops._ptr(masked2), ops._ptr(None), ops._stream())
    _lib.check(rc, "pww_inpaint_prep")
    assert torch.equal(m2, m) and _same_bits(masked2, masked)


def test_inpaint_prep_refuses_a_latent_larger_than_the_image(gpu_device):
    ops = _ops()
    img, mask = P.inpaint_inputs(8, 8, 1, 1, seed=7)
    rgb_d, mask_d = torch.from_numpy(img).to(gpu_device), torch.from_numpy(mask).to(gpu_device)
    with pytest.raises(ops.PwwHipError):
        ops.inpaint_prep(rgb_d, mask_d, 9, 8)
    with pytest.raises(ops.PwwHipError):
        ops.inpaint_prep(rgb_d, mask_d, 8, 9)


# ---- cfg_combine --------------------------------------------------------------------------------------------------------------------

CFG_SHAPES = [(1,), (255,), (257,), (2048 * 256,), (2048 * 256 + 1,), (600001,), (3, 4, 5, 7), (16, 4, 96, 96)]
GUIDANCE = [0.0, 1.0, 7.5, -2.0]
# finite everywhere in fp32: (c - u) * 7.5 + u stays far below 3.4e38
SPECIALS = {torch.float16: [65504.0, -65504.0, 0.0, -0.0, 5.96e-8, -5.96e-8, 6.0e-5, -3.0e-5, 1.0, -1.0],
            torch.bfloat16: [65504.0, -65504.0, 0.0, -0.0, 1e-40, -1e-40, 9.2e-41, 1e30, -1e30, 1.0]}
_CFG_INPUTS = {}


def _cfg_inputs(shape, dtype):
    """cond / uncond with the largest values, subnormals and signed zeros in every pairing at the head AND at the very end (the ragged
    last block, the second trip of the stride loop), random elsewhere. Built once per (shape, dtype)."""
    key = (shape, dtype)
    if key not in _CFG_INPUTS:
        n = int(np.prod(shape))
        g = torch.Generator().manual_seed(n)
        c, u = (torch.randn(n, generator=g) * 3).to(dtype), (torch.randn(n, generator=g) * 3).to(dtype)
        sp = torch.tensor(SPECIALS[dtype], dtype=torch.float32).to(dtype)
        pairs_c, pairs_u = sp.repeat_interleave(len(sp)), sp.repeat(len(sp))            # every special against every special
        if dtype == torch.bfloat16:
            assert (sp[4:7].float().abs() < 1.1754944e-38).all() and (sp[4:7] != 0).all()  # really subnormal in fp32
        pairs_c, pairs_u = pairs_c.roll(-1), pairs_u.roll(-1)                           # (a lone element is 65504 against -65504)
        k = min(n, len(pairs_c))
        c[:k], u[:k] = pairs_c[:k], pairs_u[:k]
        if n > 2 * k:
            c[n - k:], u[n - k:] = pairs_c[:k], pairs_u[:k]
        _CFG_INPUTS[key] = (c.reshape(shape), u.reshape(shape))
    return _CFG_INPUTS[key]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", CFG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cfg_combine_sizes(gpu_device, shape, dtype):
    """uncond + g * (cond - uncond) bit for bit against the oracle on the fp32 upcasts: one element, the ragged last block, exactly the
    grid cap of 2048 x 256 threads, one element past it, and 600 001 elements (the stride loop runs twice and ends ragged)."""
    ops = _ops()
    c, u = _cfg_inputs(shape, dtype)
    cd, ud = c.to(gpu_device), u.to(gpu_device)
    for g in GUIDANCE:
        want = O.cfg_combine(c.float(), u.float(), g)
        got = ops.cfg_combine(cd, ud, g)
        assert got.dtype == torch.float32 and got.shape == c.shape
        assert torch.isfinite(want).all()
        assert _same_bits(got, want.numpy()), (g, int((_bits(got) != _bits(want.numpy())).sum()))


# ---- store_f32 ----------------------------------------------------------------------------------------------------------------------

SENTINEL = 12345.678
STORE_VALUES = [-0.0, 1e-45, 3.4e38, float("inf"), float("nan"), 0.1, -2.5, float("-inf"), -1e-45, 0.0]


def _store_values(n):
    g = np.random.default_rng(n)
    return (STORE_VALUES + [float(v) for v in g.standard_normal(64)])[:n]


def _f32_bits(values):
    return np.array(values, dtype=np.float64).astype(np.float32).view(np.int32)


@pytest.mark.parametrize("n", [1, 5, 64])
def test_store_f32_writes_n_words_and_no_more(gpu_device, n):
    ops = _ops()
    buf = torch.full((96,), SENTINEL, device=gpu_device)
    values = _store_values(n)
    ops.store_f32(buf, values)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n].view(np.int32), _f32_bits(values))
    assert np.array_equal(got[n:].view(np.int32), _f32_bits([SENTINEL] * (96 - n)))


def test_store_f32_back_to_back(gpu_device):
    """Two stores on one stream, no synchronisation between: the values travel in each launch's own arguments, so both land."""
    ops = _ops()
    buf = torch.full((96,), SENTINEL, device=gpu_device)
    a, b = _store_values(5), [float(v) for v in range(100, 164)]
    ops.store_f32(buf, a)
    ops.store_f32(buf[30:], b)
    got = buf.cpu().numpy().view(np.int32)
    assert np.array_equal(got[:5], _f32_bits(a)) and np.array_equal(got[30:94], _f32_bits(b))
    assert np.array_equal(got[5:30], _f32_bits([SENTINEL] * 25)) and np.array_equal(got[94:], _f32_bits([SENTINEL] * 2))


def test_store_f32_refusals(gpu_device):
    ops = _ops()
    buf = torch.full((96,), SENTINEL, device=gpu_device)
    with pytest.raises(ops.PwwHipError):
        ops.store_f32(buf, [])
    with pytest.raises(ops.PwwHipError):
        ops.store_f32(buf, [1.0] * 65)
    assert bool((buf == SENTINEL).all())
