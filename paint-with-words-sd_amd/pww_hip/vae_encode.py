"""AutoencoderKL encode on the native path: an init image -> the scaled latent.

`encode(vae, image, noise, output, scale)` is `scale * vae.encode(image).latent_dist.sample()` (noise="sample", or a noise tensor), `scale *
.mode()` (noise=None) or, with output="moments", the pair (mean, logvar) -- in fp32, for a VAE with the encoder layout of diffusers 0.10.0
(`covers(vae)`; sd_standin.AutoencoderKLEncDec has it). The head (image -> conv_in, from the [B, 3, H, W] tensor or straight from the uint8
pixels), the three downsamplers (stride 2, padding on the right and bottom only) and the tail (conv_norm_out, SiLU, conv_out, quant_conv,
mean / logvar, clamp, the scaled sample) run on libpww_hip_vaeenc.so (include/pww_hip_vaeenc.h); between them every ResnetBlock2D and
GroupNorm runs on the kernels the UNet uses (ops.group_norm, ops.conv3x3, ops.conv3x3_shortcut) and the mid block's attention as in the
decoder (pww_hip.vae, with its PWW_VAE_ATTN switch). Wherever a `*_takes` says no, that op runs as the stock op and is counted (`stats()`).

The noise: noise="sample" draws `torch.randn(mean.shape, device=mean.device).to(mean.dtype)` -- fp32 normals from the default generator of the
VAE's device, cast to its dtype -- exactly what the stand-in's `latent_dist.sample()` draws, so the generators are left as the stock line
leaves them. Mean and std are NOT rounded to the storage type in between: the latent is fp32 from the normalised activation on.

Switches (environment, read per call): PWW_VAE_ENCODE=0 keeps `vae.encode` everywhere (`enabled()`); PWW_VAE_ENC_HEAD=0 / PWW_VAE_ENC_DOWN=0 /
PWW_VAE_ENC_TAIL=0 run the head / the downsamplers / the tail as stock ops. Defaults and the measurements behind them: profiles/vae_encode.md.
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from . import vae as V
from ._lib import PwwHipError
from .ops import _DT, _ptr, _stream

_PARTS = ("head", "group_norm", "conv3x3", "conv_shortcut", "down", "attention", "proj_attn", "tail")
_STATS = {k: [0, 0] for k in _PARTS}
_CALLS = [0]
SCALE = 0.18215
HEAD_CHANNELS, TAIL_CHANNELS, TAIL_GROUPS = _lib.VAEENC_HEAD_CHANNELS, _lib.VAEENC_TAIL_CHANNELS, _lib.VAEENC_TAIL_GROUPS


def enabled():
    """Default ON: measured, bf16, the whole native encode of a 512 x 512 image takes 3.0 ms against 9.0 ms stock (profiles/vae_encode.md)."""
    return os.environ.get("PWW_VAE_ENCODE", "1") != "0"


def head_enabled():
    """Default ON: 44.5 us at 512 x 512 against 60.7 us for the stock convolution on a channels_last input (171.6 us on an NCHW one)."""
    return os.environ.get("PWW_VAE_ENC_HEAD", "1") != "0"


def down_enabled():
    """Default ON: 35 - 43 us at the three levels of a 512 x 512 image against 80 - 81 us for F.pad + the stock convolution."""
    return os.environ.get("PWW_VAE_ENC_DOWN", "1") != "0"


def tail_enabled():
    """Default ON: 57 us at the 64 x 64 latent against 120 us for the stock op sequence."""
    return os.environ.get("PWW_VAE_ENC_TAIL", "1") != "0"


def stats():
    """{part: {"native": n, "stock": n}} since the last reset_stats(), and "encodes": the calls of `encode`. Parts: head (conv_in), group_norm
    (every norm but conv_norm_out), conv3x3 (the resnets' convolutions without a shortcut), conv_shortcut (conv2 of the resnets that have
    one), down (the downsamplers), attention (the mid block's softmax(q k^T) v), proj_attn (its output projection + residual), tail."""
    out = {k: {"native": v[0], "stock": v[1]} for k, v in _STATS.items()}
    out["encodes"] = _CALLS[0]
    return out


def reset_stats():
    for v in _STATS.values():
        v[0] = v[1] = 0
    _CALLS[0] = 0


def _count(part, native):
    _STATS[part][0 if native else 1] += 1
    return native


# ---- the structural check ------------------------------------------------------------------------------------------------------------------
def _is_down_conv(m, channels):
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (2, 2) and m.padding == (0, 0) and m.dilation == (1, 1) and m.groups == 1
            and m.padding_mode == "zeros" and m.bias is not None and m.in_channels == channels and m.out_channels == channels)


def covers(vae, require_device=True):
    """True for a float16 / bfloat16 module on a HIP device with the encoder layout of diffusers 0.10.0's AutoencoderKL: encoder.conv_in (3 x 3,
    padding 1), .down_blocks of ResnetBlock2D without a time embedding (+ .downsamplers[0].conv: 3 x 3, stride 2, padding 0 -- the module pads
    right and bottom itself), .mid_block (.resnets[0], .attentions[0] -- one head --, .resnets[1]), .conv_norm_out, .conv_out, and quant_conv
    (1 x 1) over an even number of moments. sd_standin.AutoencoderKL (no encoder), TinyVAE, an fp32 module or one on the CPU is not covered.
    require_device=False: the layout and dtype checks alone (what a host without a GPU can ask)."""
    try:
        enc, qc = vae.encoder, vae.quant_conv
        cin, mid = enc.conv_in, enc.mid_block
        w = cin.weight
        if not (w.dtype in _DT and (w.is_cuda or not require_device) and V._is_conv(cin, 3)):
            return False
        if any(p.dtype != w.dtype or p.device != w.device for m in (enc, qc) for p in m.parameters()):
            return False
        ch = cin.out_channels
        for block in enc.down_blocks:
            if getattr(block, "attentions", None):
                return False
            for r in block.resnets:
                if not (V._resnet_ok(r) and r.conv1.in_channels == ch):
                    return False
                ch = r.conv1.out_channels
            downs = getattr(block, "downsamplers", None)
            if downs is not None and not (len(downs) == 1 and _is_down_conv(getattr(downs[0], "conv", None), ch)):
                return False
        if not (len(mid.resnets) == 2 and len(mid.attentions) == 1 and all(V._resnet_ok(r) and r.conv1.in_channels == ch and r.conv1.out_channels == ch
                                                                           for r in mid.resnets) and V._attn_ok(mid.attentions[0], ch)):
            return False
        moments = qc.out_channels
        return (V._is_norm(enc.conv_norm_out, ch) and V._is_conv(enc.conv_out, 3, ch, moments) and V._is_conv(qc, 1, moments, moments)
                and moments % 2 == 0)
    except AttributeError:
        return False


# ---- the three kernels of libpww_hip_vaeenc.so ---------------------------------------------------------------------------------------------
_TABLES = {}


def pixel_table(dtype, device):
    """The 256 values a uint8 pixel normalises to, in `dtype`: the expression of paint_with_words.preprocess itself -- fp32 p / 255, times 2,
    minus 1 -- and the cast `image.to(vae.dtype)` of the call sites, so the uint8 form of the head sees the bits the tensor form is given."""
    key = (dtype, str(device))
    if key not in _TABLES:
        import numpy as np
        pixels = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0
        _TABLES[key] = (2.0 * torch.from_numpy(pixels) - 1.0).to(dtype).to(device)
    return _TABLES[key]


def _image_form(image):
    """"uint8" for a [B, H, W, 3] uint8 tensor, "sample" for a [B, 3, H, W] float16 / bfloat16 one, else None."""
    if not (torch.is_tensor(image) and image.dim() == 4):
        return None
    if image.dtype == torch.uint8:
        return "uint8" if image.shape[3] == 3 else None
    return "sample" if image.dtype in _DT and image.shape[1] == 3 else None


def head_takes(image, weight, bias):
    """True when pww_vaeenc_head_fwd runs this call: a [B, 3, H, W] float16 / bfloat16 tensor of the weight's dtype, or a [B, H, W, 3] uint8
    tensor, on a HIP device; a [128, 3, 3, 3] weight and a [128] bias in float16 / bfloat16 on that device."""
    form = _image_form(image)
    if form is None or not image.is_cuda or not (torch.is_tensor(weight) and torch.is_tensor(bias) and weight.dtype in _DT):
        return False
    B, H, W = (image.shape[0], image.shape[1], image.shape[2]) if form == "uint8" else (image.shape[0], image.shape[2], image.shape[3])
    return ((form == "uint8" or image.dtype == weight.dtype) and bias.dtype == weight.dtype and weight.device == image.device and bias.device == image.device
            and tuple(weight.shape) == (HEAD_CHANNELS, 3, 3, 3) and tuple(bias.shape) == (HEAD_CHANNELS,) and B >= 1 and H >= 1 and W >= 1
            and B * H * W * HEAD_CHANNELS < 2 ** 31)


def head(image, weight, bias):
    """conv_in on pww_vaeenc_head_fwd: the channels_last [B, 128, H, W] tensor T(conv3x3(v, weight) + bias) -- fp32 accumulation, ONE rounding
    -- for v = image ([B, 3, H, W] in T) or v = pixel_table[image] ([B, H, W, 3] uint8). The zero padding is of v."""
    if not head_takes(image, weight, bias):
        raise PwwHipError("vae_encode.head: needs a [B, 3, H, W] float16/bfloat16 or a [B, H, W, 3] uint8 image on a HIP device, a [128, 3, 3, 3] weight "
                          "and a [128] bias of one float16/bfloat16 dtype")
    form = _image_form(image)
    image = image.contiguous()
    B, H, W = (image.shape[0], image.shape[1], image.shape[2]) if form == "uint8" else (image.shape[0], image.shape[2], image.shape[3])
    table = pixel_table(weight.dtype, image.device) if form == "uint8" else None
    y = torch.empty((B, HEAD_CHANNELS, H, W), dtype=weight.dtype, device=image.device, memory_format=torch.channels_last)
    d = _lib.VaeEncHeadDesc(ctypes.sizeof(_lib.VaeEncHeadDesc), _DT[weight.dtype], B, H, W, _lib.VAEENC_IN_UINT8 if form == "uint8" else _lib.VAEENC_IN_SAMPLE)
    lib = _lib.load_vaeenc()
    with torch.cuda.device(image.device):
        _lib.check(lib.pww_vaeenc_head_fwd(_ptr(image), _ptr(table), _ptr(weight.contiguous()), _ptr(bias.contiguous()), _ptr(y), ctypes.byref(d), _stream()),
                   "pww_vaeenc_head_fwd", lib)
    return y


def head_stock(image, conv):
    """The sequence the kernel replaces: (the table lookup and the NCHW view for a uint8 image,) the stock convolution; channels_last out."""
    if image.dtype == torch.uint8:
        image = pixel_table(conv.weight.dtype, image.device)[image.long()].permute(0, 3, 1, 2)
    return V._cl(F.conv2d(image, conv.weight, conv.bias, padding=1))


def down_takes(x, weight, bias=None):
    """True when pww_vaeenc_down_fwd runs this call: a channels_last [B, Cin, H, W] float16 / bfloat16 x on a HIP device with H, W >= 2, a
    [Cout, Cin, 3, 3] weight (and a [Cout] bias) of its dtype, Cin and Cout multiples of 64."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _DT and torch.is_tensor(weight) and weight.dtype == x.dtype and weight.dim() == 4):
        return False
    B, C, H, W = x.shape
    Cout = weight.shape[0]
    return (tuple(weight.shape[1:]) == (C, 3, 3) and C % 64 == 0 and Cout % 64 == 0 and Cout >= 64 and H >= 2 and W >= 2
            and (bias is None or (torch.is_tensor(bias) and bias.dtype == x.dtype and tuple(bias.shape) == (Cout,)))
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0 and B * H * W * C < 2 ** 31 // 4)


def down(x, weight, bias=None, tile_n=0, splitk=0):
    """F.conv2d(F.pad(x, (0, 1, 0, 1)), weight, bias, stride=2) of a channels_last x -> channels_last [B, Cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1]
    on the implicit GEMM of ops.conv3x3 compiled for this geometry; epilogue T(T(conv) + bias). tile_n / splitk: 0 = the library's choice."""
    if not down_takes(x, weight, bias):
        raise PwwHipError("vae_encode.down: needs a channels_last float16/bfloat16 x with H, W >= 2, Cin, Cout multiples of 64 and a 3 x 3 weight of its dtype")
    B, C, H, W = x.shape
    Cout = weight.shape[0]
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    w = ops._khwc_weight(weight)
    d = _lib.VaeEncDownDesc(ctypes.sizeof(_lib.VaeEncDownDesc), _DT[x.dtype], B, H, W, C, Cout, int(tile_n), int(splitk))
    lib = _lib.load_vaeenc()
    y = torch.empty((B, Cout, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    nbytes = int(lib.pww_vaeenc_down_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_vaeenc_down_fwd(_ptr(x), _ptr(w), _ptr(bias.contiguous() if bias is not None else None), _ptr(y), ctypes.byref(d), _ptr(ws), nbytes,
                                           _stream()), "pww_vaeenc_down_fwd", lib)
    return y


def down_stock(x, conv):
    """The sequence the kernel replaces: pad right and bottom, the stock stride-2 convolution; channels_last out."""
    return V._cl(F.conv2d(F.pad(x, (0, 1, 0, 1)), conv.weight, conv.bias, stride=2))


def _tail_desc(x, eps, scale):
    B, C, H, W = x.shape
    return _lib.VaeEncTailDesc(ctypes.sizeof(_lib.VaeEncTailDesc), _DT[x.dtype], B, H, W, C, float(eps), float(scale))


def tail_takes(x, norm_weight, norm_bias, weight, bias, quant_weight, quant_bias, noise=None, groups=32):
    """True when pww_vaeenc_tail_fwd runs this call: a channels_last [B, 512, h, w] float16 / bfloat16 x on a HIP device, 32 groups, a [512]
    affine, a [8, 512, 3, 3] weight + [8] bias, a [8, 8(, 1, 1)] quant weight + [8] bias, and a [B, 4, h, w] noise or None, all of its dtype."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _DT and x.shape[1] == TAIL_CHANNELS and groups == TAIL_GROUPS):
        return False
    B, C, H, W = x.shape
    params = (norm_weight, norm_bias, weight, bias, quant_weight, quant_bias) + (() if noise is None else (noise,))
    return (x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0 and x.numel() < 2 ** 31 and B <= 65535
            and all(torch.is_tensor(t) and t.dtype == x.dtype and t.device == x.device for t in params)
            and tuple(norm_weight.shape) == (C,) and tuple(norm_bias.shape) == (C,) and tuple(weight.shape) == (8, C, 3, 3) and tuple(bias.shape) == (8,)
            and tuple(quant_weight.shape) in ((8, 8), (8, 8, 1, 1)) and tuple(quant_bias.shape) == (8,)
            and (noise is None or tuple(noise.shape) == (B, 4, H, W)))


def tail_statistics(x, eps=1e-6):
    """The statistics launch alone: the fp32 [B, chunks, 32, 2] per-chunk (sum, sum of squares) of a channels_last [B, 512, h, w] x, as the
    fused launch reads them. Bitwise repeatable."""
    e = x.new_empty
    if not (torch.is_tensor(x) and x.dim() == 4 and tail_takes(x, e(512), e(512), e(8, 512, 3, 3), e(8), e(8, 8), e(8))):
        raise PwwHipError("vae_encode.tail_statistics: needs a channels_last [B, 512, h, w] float16/bfloat16 tensor on a HIP device")
    d = _tail_desc(x, eps, 1.0)
    lib = _lib.load_vaeenc()
    nbytes, chunks = int(lib.pww_vaeenc_tail_workspace_bytes(ctypes.byref(d))), int(lib.pww_vaeenc_tail_chunks(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_vaeenc_tail_stats(_ptr(x), None, ctypes.byref(d), _ptr(ws), nbytes, _stream()), "pww_vaeenc_tail_stats", lib)
    return ws[:x.shape[0] * chunks * 64].view(x.shape[0], chunks, 32, 2)


def tail(x, norm_weight, norm_bias, weight, bias, quant_weight, quant_bias, noise=None, eps=1e-6, scale=SCALE, moments=True):
    """m = quant(conv3x3(silu(group_norm_32(x)), weight) + bias) of a channels_last [B, 512, h, w] x in two launches -> (moments, z), both fp32:
    moments [B, 8, h, w] = mean | clamp(logvar, -30, 20) (None with moments=False), z [B, 4, h, w] = scale * (mean + exp(logvar / 2) * noise),
    or scale * mean for noise=None. fp32 from the norm to the outputs."""
    if not tail_takes(x, norm_weight, norm_bias, weight, bias, quant_weight, quant_bias, noise):
        raise PwwHipError("vae_encode.tail: needs a channels_last [B, 512, h, w] float16/bfloat16 x on a HIP device, a [512] affine, a [8, 512, 3, 3] weight, "
                          "a [8] bias, a [8, 8] quant weight, a [8] quant bias and a [B, 4, h, w] noise (or None) of its dtype")
    B, C, H, W = x.shape
    d = _tail_desc(x, eps, scale)
    lib = _lib.load_vaeenc()
    nbytes = int(lib.pww_vaeenc_tail_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    mom = torch.empty((B, 8, H, W), dtype=torch.float32, device=x.device) if moments else None
    z = torch.empty((B, 4, H, W), dtype=torch.float32, device=x.device)
    args = [t.contiguous() for t in (norm_weight, norm_bias, weight, bias, quant_weight, quant_bias)]
    noise = noise.contiguous() if noise is not None else None
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_vaeenc_tail_fwd(_ptr(x), *[_ptr(t) for t in args], _ptr(noise), _ptr(mom), _ptr(z), ctypes.byref(d), _ptr(ws), nbytes, _stream()),
                   "pww_vaeenc_tail_fwd", lib)
    return mom, z


def tail_stock(x, norm, conv, quant_conv, noise=None, scale=SCALE):
    """The sequence the kernel replaces, in x's dtype: group_norm, silu, conv_out, quant_conv, chunk, clamp, exp, the sample -> (moments, z) as
    `tail` returns them (cast to fp32 at the end, as the call sites cast the sample)."""
    m = quant_conv(conv(F.silu(F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps))))
    mean, logvar = torch.chunk(m, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    z = mean if noise is None else mean + torch.exp(0.5 * logvar) * noise
    return torch.cat([mean, logvar], 1).float().contiguous(), scale * z.float().contiguous()


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------
def draw_noise(shape, dtype, device):
    """The noise of the stand-in's `latent_dist.sample()` (generator=None): fp32 normals from the device's default generator, cast to `dtype`."""
    return torch.randn(shape, generator=None, device=device).to(dtype)


def encode(vae, image, noise=None, output="latent", scale=SCALE):
    """The fp32 latent `scale * (mean + std * noise)` ([B, 4, H / 8, W / 8]) of a VAE `covers()` accepts, or with output="moments" the fp32 pair
    (mean, logvar). image: [B, 3, H, W] in the VAE's dtype (what `vae.encode` is given; another float dtype is cast), or the [B, H, W, 3] uint8
    pixels themselves; H and W multiples of 8. noise: a [B, 4, H / 8, W / 8] tensor, "sample" (drawn as `latent_dist.sample()` draws it), or
    None (the mode)."""
    if output not in ("latent", "moments"):
        raise PwwHipError("vae_encode.encode: output must be 'latent' or 'moments'")
    if not covers(vae):
        raise PwwHipError("vae_encode.encode: the module has not the AutoencoderKL encoder layout in float16/bfloat16 on a HIP device (pww_hip.vae_encode.covers)")
    enc = vae.encoder
    dtype, dev = enc.conv_in.weight.dtype, enc.conv_in.weight.device
    if not (torch.is_tensor(image) and image.dim() == 4):
        raise PwwHipError("vae_encode.encode: image must be a [B, 3, H, W] tensor or a [B, H, W, 3] uint8 tensor")
    if image.dtype != torch.uint8:
        image = image.to(dtype)
    if _image_form(image) is None:
        raise PwwHipError("vae_encode.encode: image must be a [B, 3, H, W] tensor or a [B, H, W, 3] uint8 tensor")
    image = image.to(dev)
    B, H, W = (image.shape[0], image.shape[1], image.shape[2]) if image.dtype == torch.uint8 else (image.shape[0], image.shape[2], image.shape[3])
    if H % 8 or W % 8:
        raise PwwHipError("vae_encode.encode: H and W must be multiples of 8 (got %d x %d)" % (H, W))
    lat = (B, vae.quant_conv.out_channels // 2, H // 8, W // 8)
    if torch.is_tensor(noise):
        if tuple(noise.shape) != lat:
            raise PwwHipError("vae_encode.encode: noise must be %s (got %s)" % (lat, tuple(noise.shape)))
    elif noise is not None and noise != "sample":
        raise PwwHipError("vae_encode.encode: noise must be a tensor, 'sample' or None")
    _CALLS[0] += 1
    with torch.no_grad(), V.counting(_STATS):
        cin = enc.conv_in
        if _count("head", head_enabled() and head_takes(image, cin.weight, cin.bias)):
            x = head(image, cin.weight, cin.bias)
        else:
            x = head_stock(image, cin)
        for block in enc.down_blocks:
            for r in block.resnets:
                x = V._resnet(r, x)
            if getattr(block, "downsamplers", None) is not None:
                conv = block.downsamplers[0].conv
                if _count("down", down_enabled() and down_takes(x, conv.weight, conv.bias)):
                    x = down(x, conv.weight, conv.bias)
                else:
                    x = down_stock(x, conv)
        mid = enc.mid_block
        x = V._resnet(mid.resnets[0], x)
        x = V._attention_block(mid.attentions[0], x)
        x = V._resnet(mid.resnets[1], x)
        x = x.contiguous(memory_format=torch.channels_last)
        # the noise is drawn HERE, where `latent_dist.sample()` draws it: after the encoder ran
        if torch.is_tensor(noise):
            noise = noise.to(device=dev, dtype=dtype)
        elif noise == "sample":
            noise = draw_noise(lat, dtype, dev)
        norm, conv, qc = enc.conv_norm_out, enc.conv_out, vae.quant_conv
        if _count("tail", tail_enabled() and tail_takes(x, norm.weight, norm.bias, conv.weight, conv.bias, qc.weight, qc.bias, noise, norm.num_groups)):
            moments, z = tail(x, norm.weight, norm.bias, conv.weight, conv.bias, qc.weight, qc.bias, noise, norm.eps, scale, moments=output == "moments")
        else:
            moments, z = tail_stock(x, norm, conv, qc, noise, scale)
    if output == "moments":
        half = moments.shape[1] // 2
        return moments[:, :half], moments[:, half:]
    return z
