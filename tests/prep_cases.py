"""Shapes and seeded synthetic inputs of the request-preparation kernels' edge tests (csrc/pww_mask.hip), shared by the GPU tests
(test_prep_kernels_gpu.py: kernel vs oracle) and the host test that holds the oracle to torch at the same shapes
(test_oracle_shapes_host.py). Test infrastructure."""
import numpy as np

from oracle import pww_oracle as O

DEFAULT_RATIOS = (8, 16, 32, 64)

# (H, W) of the colour maps. 32 x 32: levels of 16 / 4 / 1 / 1 pixels, every one under a workgroup, Hr == Wr == 1 twice.
# 40 x 72: non-square, 3 x 5 at ratio 16 by half-up rounding. 100 x 36: 13 x 5 = 65 pixels at ratio 8 (a full workgroup + 1),
# Wr == 1 from ratio 32 on. 36 x 100: its transpose.
MASK_SHAPES = [(32, 32), (40, 72), (100, 36), (36, 100)]
RATIO_SHAPE = (40, 72)                                              # the map of the non-default ratio sets
RATIO_SETS = [(1,), (8, 16), (8, 16, 32, 64, 4)]

# (H, W, T, n_tokens) of the _ORIG fallback resize
RESIZE_CASES = [(16, 16, 77, 256),      # oh * ow == n
                (16, 16, 3, 200),       # oh * ow = 196 < n: the 1-D nearest step repeats entries
                (20, 12, 5, 60),
                (9, 33, 1, 4),          # oh == 1
                (33, 9, 2, 4),          # ow == 1
                (8, 8, 77, 1)]          # one token: oh == ow == 1
RESIZE_REFUSED = (8, 8, 4, 65)          # n_tokens > H * W

# (H, W, h, w) of the inpainting inputs
# (the first six: scales H / h and W / w equal or close, 8.25 and 8.75 at the most apart; the last: 12 against 5)
INPAINT_CASES = [(8, 8, 1, 1), (500, 500, 62, 62), (40, 72, 5, 9), (72, 40, 9, 5), (17, 31, 17, 31), (33, 35, 4, 4), (48, 40, 4, 8)]

BLUR_SIZES = [(20, 20), (20, 57), (57, 21)]                         # ksize 39; 20 = ksize / 2 + 1 is the smallest legal side
BLUR_SMALL = ((9, 64), 5)                                           # (size, ksize)
BLUR_SIGMAS = [0.3, 4.0, 25.0]


ABSENT = (1, 2, 3)                      # a colour no palette holds


def level_size(H, W, ratio):
    return O.always_round(H / ratio), O.always_round(W / ratio)


def palette(R, seed=0):
    """R distinct colours; ABSENT is none of them."""
    g = np.random.default_rng(1000 + seed)
    seen, out = {ABSENT}, []
    while len(out) < R:
        c = tuple(int(v) for v in g.integers(0, 256, size=3))
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def strengths(R):
    """0.05, 0.15, ...: none representable in binary, all distinct, so the order of the fp32 additions shows in the sum."""
    return [0.1 * k + 0.05 for k in range(R)]


def colour_map(H, W, colours, seed, cell):
    """A map of `colours` in cells of `cell` (3 or 5) pixels, so that cell edges fall inside every ratio's bilinear footprint."""
    g = np.random.default_rng(seed)
    idx = g.integers(0, len(colours), size=(-(-H // cell), -(-W // cell)))
    idx = np.kron(idx, np.ones((cell, cell), dtype=idx.dtype))[:H, :W]
    return np.ascontiguousarray(np.array(colours, dtype=np.uint8)[idx])


def region_masks(rgb, colours, strength):
    """fp32 [R, H, W]: strength_r where the pixel has colour r (what separate_regions builds, :231-236)."""
    return np.stack([(rgb == np.array(c, np.uint8)[None, None, :]).all(-1).astype(np.float32) * np.float32(s)
                     for c, s in zip(colours, strength)])


def prompt(kind, R, T):
    """(per-region phrase ids, token_ids of length T) of one hand-built prompt.
    all:    every region has the phrase [7], which stands at one position: that position collects all R regions, in region order.
    mixed:  region 0's phrase [5, 6] occurs twice (three more times in a long prompt, once as its last two positions); regions 1 and 2
            share the phrase [9]; every other region r has [100 + r], placed while there is room; the positions between collect nothing.
    none:   no phrase occurs: every column list is empty."""
    tok = [0] * T
    if kind == "all":
        tok[min(3, T - 1)] = 7
        return [[7] for _ in range(R)], tok
    if kind == "none":
        return [[100 + r] for r in range(R)], tok
    assert kind == "mixed"
    if T == 1:
        return [[5]] + [[100 + r] for r in range(1, R)], [5]
    ids = [[5, 6]] + [[9] if r in (1, 2) else [100 + r] for r in range(1, R)]
    seq = [5, 6, 0, 9, 0, 5, 6, 9, 0] + [v for r in range(3, R) for v in (100 + r, 0)]
    tok = (seq + [0] * T)[:T]
    if T > 140:
        tok[135:137] = [5, 6]
        tok[T - 2:] = [5, 6]
        tok[T - 9] = 9
    return ids, tok


def random_weights(H, W, T, seed):
    return (np.random.default_rng(seed).random((H, W, T), dtype=np.float32) * np.float32(1.5)).astype(np.float32)


def nearest_grid(n_in, n_out):
    """The source index of every output index of a nearest resize, in exact integers: floor(o * n_in / n_out)."""
    return [(o * n_in) // n_out for o in range(n_out)]


def inpaint_inputs(H, W, h, w, seed):
    """uint8 image [H, W, 3] with 0 and 255 present and uint8 mask [H, W]. The pixels the nearest resize to (h, w) samples hold 127 and
    128, the two sides of the 0.5 threshold, as a checkerboard over the latent grid -- so the latent mask is that checkerboard, and a
    kernel that samples any other pixel reads a random byte. Every other pixel draws from all 256 byte values (each present where 256
    pixels are free). Where the resize samples nearly every pixel (h == H) only every second latent row and column is placed."""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    img[0, 0, 0], img[0, 0, 1], img[H - 1, W - 1, 2] = 0, 255, 0
    mask = np.zeros((H, W), np.uint8)
    fixed = np.zeros((H, W), bool)
    step = 1 if H * W - h * w >= 256 or H * W < 256 else 2
    ys, xs = nearest_grid(H, h), nearest_grid(W, w)
    for i in range(0, h, step):
        for j in range(0, w, step):
            mask[ys[i], xs[j]], fixed[ys[i], xs[j]] = 127 + ((i // step + j // step) & 1), True
    free = np.resize(np.arange(256, dtype=np.uint8), int((~fixed).sum()))
    g.shuffle(free)
    mask[~fixed] = free
    return img, mask


def blur_mask(H, W, seed):
    """0 / 1.5 valued, like the product's strength-scaled region masks."""
    return (np.random.default_rng(seed).random((H, W)) < 0.4).astype(np.float32) * np.float32(1.5)
