"""The oracle's resize / blur restatements (oracle/pww_oracle.py) against torch at the edge shapes of tests/test_prep_kernels_gpu.py.

test_oracle_golden.py pins the oracle to the reference's outputs at product sizes (512 x 512 and the like). The GPU edge tests hold
the kernels of csrc/pww_mask.hip to the oracle bit for bit at 1-pixel levels, non-square maps, one-token resizes and the smallest
legal blur -- shapes the goldens never reach. Here the oracle itself is held to the ATen operators the reference calls, at exactly
those shapes (tests/prep_cases.py). CPU only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prep_cases as P
from gpu_util import _blur_exact
from oracle import pww_oracle as O


def _levels():
    out = []
    for H, W in P.MASK_SHAPES:
        out += [(H, W) + P.level_size(H, W, r) for r in P.DEFAULT_RATIOS]
    out += [P.RATIO_SHAPE + P.level_size(*P.RATIO_SHAPE, r) for r in (1, 4)]
    for H, W, _, n in P.RESIZE_CASES:                 # the intermediate size of the _ORIG fallback
        s = 1 / math.sqrt(H * W / n)
        out.append((H, W, int(math.floor(H * s)), int(math.floor(W * s))))
    return sorted(set(out))


@pytest.mark.parametrize("H,W,oh,ow", _levels(), ids=lambda v: str(v))
def test_bilinear_resize_matches_torch(H, W, oh, ow):
    """bilinear(align_corners=True) of a strength-scaled cell map (values <= 1.5) vs F.interpolate: <= 1e-6, the bar of
    test_mask_weights_match_reference (ATen contracts the lerp into FMAs, the oracle keeps the plain fp32 formula)."""
    colours = P.palette(5)
    rgb = P.colour_map(H, W, colours, seed=H * 1000 + W, cell=3)
    for mask in P.region_masks(rgb, colours, [0.3, 0.7, 1.0, 1.3, 1.5]):
        want = F.interpolate(torch.from_numpy(mask)[None, None], size=(oh, ow), mode="bilinear", align_corners=True)[0, 0].numpy()
        got = O.bilinear_resize(mask, oh, ow, align_corners=True)
        assert got.shape == want.shape == (oh, ow)
        err = np.abs(got - want).max()
        print(f"bilinear {H}x{W} -> {oh}x{ow}: max abs err {err:.2e}")
        assert err <= 1e-6


@pytest.mark.parametrize("H,W,h,w", P.INPAINT_CASES)
def test_nearest_resize_matches_torch(H, W, h, w):
    """The latent-size mask: exactly F.interpolate(mode='nearest'), where the fp32 floor(y * H / h) lands next to an integer too."""
    _, mask = P.inpaint_inputs(H, W, h, w, seed=7)
    m, _ = O.prepare_mask_and_masked_image(np.zeros((H, W, 3), np.uint8), mask)
    want = F.interpolate(m, size=(h, w))                   # (the default mode is 'nearest')
    got = O.nearest_resize(m.numpy(), h, w)
    assert np.array_equal(got, want.numpy())
    # and on a map whose value IS the source index, so that a neighbouring source pixel cannot give the same answer
    idx = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    assert np.array_equal(O.nearest_resize(idx.numpy(), h, w), F.interpolate(idx, size=(h, w)).numpy())


@pytest.mark.parametrize("H,W,T,n", P.RESIZE_CASES)
def test_orig_weight_fallback_matches_torch(H, W, T, n):
    """The two torch calls of the reference's fallback (scale_factor bilinear, align_corners=True; then 1-D nearest to n): <= 1e-6."""
    w = P.random_weights(H, W, T, seed=n)
    t = torch.from_numpy(w).permute(2, 0, 1)[None]
    small = F.interpolate(t, scale_factor=1 / math.sqrt(H * W / n), mode="bilinear", align_corners=True)
    want = F.interpolate(small.reshape(1, T, -1), size=n, mode="nearest")[0].t().numpy()
    got = O.orig_weight_fallback(w, n)
    assert got.shape == want.shape == (n, T)
    err = np.abs(got - want).max()
    print(f"_ORIG fallback {H}x{W}x{T} -> {n}: intermediate {tuple(small.shape[-2:])}, max abs err {err:.2e}")
    assert err <= 1e-6


@pytest.mark.parametrize("sigma", P.BLUR_SIGMAS)
def test_gaussian_blur_matches_exact_at_the_smallest_size(sigma):
    """20 x 20 at ksize 39: the reflection reaches index 0 and index 19 from both sides. Bar 5e-6, the oracle conv's own rounding noise
    (test_round2_gpu.py::test_gauss_blur_kernel)."""
    m = P.blur_mask(20, 20, seed=3)
    err = np.abs(O.gaussian_blur(m, sigma) - _blur_exact(m, sigma)).max()
    print(f"oracle blur 20x20 sigma {sigma}: max abs err vs fp64 {err:.2e}")
    assert err <= 5e-6


@pytest.mark.parametrize("sigma", P.BLUR_SIGMAS)
def test_gaussian_blur_takes_another_ksize(sigma):
    """ksize 5 on 9 x 64: the oracle's ksize argument agrees with the fp64 convolution, so the GPU test may use both."""
    (H, W), ks = P.BLUR_SMALL
    m = P.blur_mask(H, W, seed=4)
    err = np.abs(O.gaussian_blur(m, sigma, ks) - _blur_exact(m, sigma, ks)).max()
    print(f"oracle blur {H}x{W} ksize {ks} sigma {sigma}: max abs err vs fp64 {err:.2e}")
    assert err <= 5e-6


def test_inputs_are_what_the_cases_claim():
    """The synthetic inputs themselves: the prompts' column lists and the masks' byte values."""
    ids, tok = P.prompt("all", 64, 77)
    regions = [(i, np.zeros((2, 2), np.float32)) for i in ids]
    cols = O.column_region_lists(regions, tok)
    assert cols[3] == list(range(64)) and sum(len(c) for c in cols) == 64
    for T in (77, 231):
        ids, tok = P.prompt("mixed", 64, T)
        cols = O.column_region_lists([(i, np.zeros((2, 2), np.float32)) for i in ids], tok)
        assert len(tok) == T and cols[0] == [0] and cols[1] == [0] and cols[5] == [0] and cols[3] == [1, 2] and cols[2] == []
    assert cols[T - 1] == [0] and cols[T - 2] == [0] and cols[136] == [0] and cols[T - 9] == [1, 2]
    assert all(len(c) == 0 for c in O.column_region_lists([(i, None) for i in P.prompt("none", 5, 77)[0]], P.prompt("none", 5, 77)[1]))
    f = np.float32
    for H, W, h, w in P.INPAINT_CASES:
        img, mask = P.inpaint_inputs(H, W, h, w, seed=7)
        assert img.min() == 0 and img.max() == 255
        ys, xs = P.nearest_grid(H, h), P.nearest_grid(W, w)
        # the integer grid the inputs are placed on IS the grid the fp32 formula of the resize samples, at every one of these shapes
        assert ys == np.floor(np.arange(h, dtype=f) * (f(H) / f(h))).astype(int).tolist()
        assert xs == np.floor(np.arange(w, dtype=f) * (f(W) / f(w))).astype(int).tolist()
        sampled = mask[np.ix_(ys, xs)].astype(int)
        if (H, W) != (h, w):             # every sampled pixel holds 127 or 128, as a checkerboard over the latent grid
            assert np.array_equal(sampled, 127 + (np.add.outer(np.arange(h), np.arange(w)) & 1))
        else:
            assert np.array_equal(sampled[::2, ::2], 127 + (np.add.outer(np.arange(0, h, 2) // 2, np.arange(0, w, 2) // 2) & 1))
        if H * W - h * w >= 256:
            assert len(np.unique(mask)) == 256
        # columns sampled with the rows' scale (sx from H / h) give another latent mask wherever the two scales differ
        m, _ = O.prepare_mask_and_masked_image(img, mask)
        xs_rows_scale = np.minimum(np.floor(np.arange(w, dtype=f) * (f(H) / f(h))).astype(int), W - 1)
        swapped = m.numpy()[0, 0][np.ix_(ys, xs_rows_scale)]
        assert (H * w == W * h) == np.array_equal(swapped, O.nearest_resize(m.numpy(), h, w)[0, 0]), (H, W, h, w)
    assert [P.level_size(40, 72, 16), P.level_size(100, 36, 8), P.level_size(100, 36, 32), P.level_size(32, 32, 64)] == [(3, 5), (13, 5), (3, 1), (1, 1)]
