"""Inputs, references and bars of the AutoencoderKL encode tests (test_vaeenc_host.py, test_vaeenc_kernels_gpu.py, test_vaeenc_encode_gpu.py and
the child process vaeenc_encode_child.py).

The reference everywhere is stock torch on the same (rounded) weights and inputs, upcast: fp64 on the CPU for the three kernels, fp32 on the
device for the whole encoder. The rule of every comparison is the one of the decode tests (vae_cases.py):

    err(native vs reference) <= 1.5 * err(stock same-dtype op sequence vs reference) + 2e-3 * max|reference|

measured per case against the stock path, never against the code under test, and per output block (mean, logvar, z) where there are several:
a large exp(logvar / 2) * noise term must not hide the mean.
"""
import copy
import functools

import torch
import torch.nn.functional as F

SCALE = 0.18215
HEAD_SHAPES = ((1, 1, 1), (1, 8, 8), (1, 24, 40), (2, 64, 64))            # (B, H, W): one pixel; less than a 16-pixel group ... ; ragged; 512 groups, 2 images
HEAD_VARIANTS = ("plain", "border")
DOWN_SHAPES = ((1, 2, 2, 128), (1, 7, 9, 128), (2, 16, 24, 256), (1, 8, 8, 512))      # (B, H, W, C): the smallest; odd (no padding read); 2 images, ragged M; deep K
DOWN_VARIANTS = ("plain", "ring")
TAIL_SHAPES = ((1, 1, 1), (1, 8, 8), (2, 5, 7), (2, 64, 64))             # (B, h, w): one pixel; one tile; ragged, 2 images; 64 tiles and 64 chunks per image
TAIL_VARIANTS = ("mode", "sample", "border", "clamp")
ENCODE_IMAGES = ((1, 3, 64, 64), (2, 3, 64, 96))
ODD_IMAGE = (1, 3, 40, 56)          # 10 x 14 and 5 x 7 at the two coarsest levels: no multiple of 8 pixels


def bar(stock, ref):
    ref = ref.double().cpu()
    return 1.5 * (stock.double().cpu() - ref).abs().max().item() + 2e-3 * ref.abs().max().item()


def check(native, stock, ref, what):
    """One output block under the rule above; prints the figures before it asserts. Returns the bar."""
    eps = bar(stock, ref)
    err = (native.double().cpu() - ref.double().cpu()).abs().max().item()
    peak = ref.abs().max().item()
    print("%s: err %.3e, bar %.3e (stock err %.3e, max|ref| %.3e)" % (what, err, eps, (eps - 2e-3 * peak) / 1.5, peak))
    assert tuple(native.shape) == tuple(ref.shape), (what, native.shape, ref.shape)
    assert err <= eps, (what, err, eps)
    return eps


def uint8_image(B, H, W):
    """[B, H, W, 3] uint8 walking through all 256 values (every one of them occurs from 86 pixels on)."""
    n = B * H * W * 3
    return ((torch.arange(n, dtype=torch.int64) * 37 + 11) % 256).to(torch.uint8).reshape(B, H, W, 3)


def pixel_table(dtype):
    """2 * (p / 255) - 1 in fp32, cast: restated (the package's own table is what the test compares with)."""
    return (2.0 * (torch.arange(256, dtype=torch.float32) / 255.0) - 1.0).to(dtype)


# ---- head ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_inputs(B, H, W, variant, dtype):
    """The uint8 image [B, H, W, 3], its [B, 3, H, W] normalised form in `dtype`, conv_in's weight [128, 3, 3, 3] and bias [128] in `dtype`.
    border: an all-black image (every value -1), so that padding with PIXEL 0 (value -1) instead of the value 0 moves every border pixel."""
    g = torch.Generator().manual_seed(311 + 17 * H + W + B)
    u8 = uint8_image(B, H, W) if variant == "plain" else torch.zeros(B, H, W, 3, dtype=torch.uint8)
    image = pixel_table(dtype)[u8.long()].permute(0, 3, 1, 2).contiguous()
    w = torch.randn(128, 3, 3, 3, generator=g) * 0.2
    bias = 0.1 * torch.randn(128, generator=g)
    return u8, image, w.to(dtype), bias.to(dtype)


@functools.lru_cache(maxsize=None)
def head_reference(B, H, W, variant, dtype):
    """fp64 on the CPU: [B, 128, H, W]."""
    _, image, w, bias = head_inputs(B, H, W, variant, dtype)
    return F.conv2d(image.double(), w.double(), bias.double(), padding=1)


def head_trap(B, H, W, variant, dtype):
    """What padding with pixel 0 (value -1) would give."""
    _, image, w, bias = head_inputs(B, H, W, variant, dtype)
    return F.conv2d(F.pad(image.double(), (1, 1, 1, 1), value=-1.0), w.double(), bias.double())


# ---- down ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def down_inputs(B, H, W, C, variant, dtype):
    """x [B, C, H, W] (NCHW on the CPU), w [C, C, 3, 3], bias [C] in `dtype`. ring: the outermost ring of pixels is brighter by 4, so reading a
    padding zero where the ring is (the symmetric padding of the UNet's downsampler), or the ring where the padding is, moves the border outputs."""
    g = torch.Generator().manual_seed(733 + 19 * H + W + B + C)
    x = torch.randn(B, C, H, W, generator=g)
    if variant == "ring":
        ring = torch.ones(H, W, dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        x[:, :, ring] += 4.0
    w = torch.randn(C, C, 3, 3, generator=g) * (9 * C) ** -0.5
    bias = 0.1 * torch.randn(C, generator=g)
    return x.to(dtype), w.to(dtype), bias.to(dtype)


@functools.lru_cache(maxsize=None)
def down_reference(B, H, W, C, variant, dtype):
    """fp64 on the CPU: the padded stride-2 convolution, [B, C, (H - 2) // 2 + 1, (W - 2) // 2 + 1]."""
    x, w, bias = (t.double() for t in down_inputs(B, H, W, C, variant, dtype))
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)


def down_trap(B, H, W, C, variant, dtype):
    """The symmetric form (padding 1 on every side), cut to the reference's size."""
    x, w, bias = (t.double() for t in down_inputs(B, H, W, C, variant, dtype))
    ref = down_reference(B, H, W, C, variant, dtype)
    return F.conv2d(x, w, bias, stride=2, padding=1)[:, :, :ref.shape[2], :ref.shape[3]]


# ---- tail ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_inputs(B, H, W, variant, dtype):
    """x [B, 512, H, W] (NCHW on the CPU), gamma, beta [512], w [8, 512, 3, 3], bias [8], qw [8, 8, 1, 1], qb [8], noise [B, 4, H, W] in `dtype`.
    border: as the decoder's tail -- the image sits at -2 with a spread of 0.25 and its border ring one higher, so that a zero of the INPUT would
    be about +8 after the norm. clamp: conv_out scaled so that logvar passes both -30 and 20."""
    g = torch.Generator().manual_seed(1499 + 13 * H + W + B)
    x = torch.randn(B, 512, H, W, generator=g)
    if variant == "border":
        x = x * 0.25 - 2.0
        ring = torch.ones(H, W, dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        x[:, :, ring] += 1.0
    x = x + 0.3 * torch.randn(B, 512, 1, 1, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)
    w = torch.randn(8, 512, 3, 3, generator=g) * (1.2 if variant == "clamp" else 0.02)
    bias = 0.1 * torch.randn(8, generator=g)
    qw = (torch.eye(8) + 0.2 * torch.randn(8, 8, generator=g)).reshape(8, 8, 1, 1)
    qb = 0.1 * torch.randn(8, generator=g)
    noise = torch.randn(B, 4, H, W, generator=g)
    return tuple(t.to(dtype) for t in (x, gamma, beta, w, bias, qw, qb, noise))


@functools.lru_cache(maxsize=None)
def tail_reference(B, H, W, variant, dtype, eps=1e-6):
    """fp64 on the CPU: (mean, logvar, z of the mode form, z of the sample form), each [B, 4, H, W]."""
    x, gamma, beta, w, bias, qw, qb, noise = (t.double() for t in tail_inputs(B, H, W, variant, dtype))
    m = F.conv2d(F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, eps)), w, bias, padding=1), qw, qb)
    mean, logvar = torch.chunk(m, 2, dim=1)
    logvar = logvar.clamp(-30.0, 20.0)
    return mean, logvar, SCALE * mean, SCALE * (mean + torch.exp(0.5 * logvar) * noise)


def tail_trap(B, H, W, variant, dtype, eps=1e-6):
    """The mean with the INPUT padded by zeros instead of the activation."""
    x, gamma, beta, w, bias, qw, qb, _ = (t.double() for t in tail_inputs(B, H, W, variant, dtype))
    mu = x.reshape(B, 32, -1).mean(-1)[:, :, None, None, None]
    var = x.reshape(B, 32, -1).var(-1, unbiased=False)[:, :, None, None, None]
    a = ((F.pad(x, (1, 1, 1, 1)).reshape(B, 32, 16, H + 2, W + 2) - mu) / (var + eps).sqrt()).reshape(B, 512, H + 2, W + 2)
    m = F.conv2d(F.conv2d(F.silu(a * gamma[None, :, None, None] + beta[None, :, None, None]), w, bias), qw, qb)
    return m[:, :4]


# ---- the whole encoder ---------------------------------------------------------------------------------------------------------------------
def make_vae(dtype, device):
    from sd_standin import AutoencoderKLEncDec
    return AutoencoderKLEncDec().to(device=device, dtype=dtype).eval()


def image(shape, dtype, device):
    """A [B, 3, H, W] image in [-1, 1]: smooth structure plus pixel noise, as normalised 8-bit values."""
    g = torch.Generator().manual_seed(77 + shape[2] * 31 + shape[3])
    low = torch.randn(shape[0], 3, max(shape[2] // 8, 1), max(shape[3] // 8, 1), generator=g)
    img = F.interpolate(low, size=shape[2:], mode="bilinear", align_corners=False) * 0.25 + 0.5 + 0.05 * torch.randn(*shape, generator=g)
    u8 = (img.clamp(0, 1) * 255).round().to(torch.uint8)
    return pixel_table(dtype)[u8.long()].to(device)


def latent_noise(shape, dtype, device):
    g = torch.Generator().manual_seed(91 + shape[2] + shape[3])
    return torch.randn(shape[0], 4, shape[2] // 8, shape[3] // 8, generator=g).to(device=device, dtype=dtype)


def encode_checks(vae, shape, dtype, device):
    """One image: pww_hip.vae_encode.encode (the latent on given noise, and the moments) against the fp32 encoder on the same weights, upcast,
    under the bars above, per block; returns stats() of the two native calls."""
    from pww_hip import vae_encode as E
    x, n = image(shape, dtype, device), latent_noise(shape, dtype, device)
    with torch.no_grad():
        ref = copy.deepcopy(vae).float().encode(x.float()).latent_dist
        ref_z = SCALE * (ref.mean + ref.std * n.float())
        stock = vae.encode(x).latent_dist
        stock_z = SCALE * (stock.mean + stock.std * n)
    E.reset_stats()
    z = E.encode(vae, x, noise=n)
    mean, logvar = E.encode(vae, x, output="moments")
    st = E.stats()
    what = "encode %s %s" % (tuple(shape), str(dtype).split(".")[-1])
    assert z.dtype == mean.dtype == logvar.dtype == torch.float32 and tuple(z.shape) == (shape[0], 4, shape[2] // 8, shape[3] // 8)
    check(mean, stock.mean, ref.mean, what + " mean")
    check(logvar, stock.logvar, ref.logvar, what + " logvar")
    check(z, stock_z, ref_z, what + " z")
    return st


# 10 resnets (2 in each of the 4 down blocks, 2 in the mid block), 2 of them with a shortcut (128 -> 256, 256 -> 512); 2 norms each + the attention's
SD_COUNTS = {"resnet_plain": 8, "resnet_shortcut": 2, "down": 3, "norms": 2 * 10 + 1}


def assert_native(st, calls, attn=True, head=True, down=True, tail=True, norms_native=None):
    """`calls` encodes of the SD configuration with everything on the native path (but what a switch turned off)."""
    on = lambda flag, n=calls: {"native": n, "stock": 0} if flag else {"native": 0, "stock": n}      # noqa: E731
    assert st["encodes"] == calls
    assert st["head"] == on(head) and st["tail"] == on(tail) and st["down"] == on(down, calls * SD_COUNTS["down"]), st
    assert st["conv3x3"] == {"native": calls * (2 * SD_COUNTS["resnet_plain"] + SD_COUNTS["resnet_shortcut"]), "stock": 0}, st
    assert st["conv_shortcut"] == {"native": calls * SD_COUNTS["resnet_shortcut"], "stock": 0}, st
    native = SD_COUNTS["norms"] if norms_native is None else norms_native
    assert st["group_norm"] == {"native": calls * native, "stock": calls * (SD_COUNTS["norms"] - native)}, st
    assert st["attention"] == on(attn), st
    assert st["proj_attn"]["native"] + st["proj_attn"]["stock"] == calls, st
