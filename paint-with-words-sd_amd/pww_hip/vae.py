"""AutoencoderKL decode on the native path: latents -> `.sample` or the 8-bit image.

`decode(vae, z, output)` is `vae.decode(z).sample` (output="sample") or, with output="uint8", the [B, H, W, 3] uint8 image
`round(255 * clamp(sample / 2 + 0.5, 0, 1))` that `_pil_from_latents` hands to PIL -- for a VAE with the decoder layout of diffusers 0.10.0
(`covers(vae)`; sd_standin.AutoencoderKL has it). post_quant_conv and conv_in stay stock ops; from there the tensor is channels_last and every
ResnetBlock2D, upsampler and GroupNorm runs on the kernels the UNet uses (ops.group_norm, ops.conv3x3, ops.conv3x3_shortcut), the mid
block's one-head attention of head dim 512 on pww_vae_attn_fwd and the tail (conv_norm_out, SiLU, conv_out, image) on pww_vae_tail_fwd
(libpww_hip_vae.so, include/pww_hip_vae.h). Wherever a `*_takes` says no, that op runs as the stock op and is counted (`stats()`).

Switches (environment, read per call): PWW_VAE=0 keeps `vae.decode` everywhere (`enabled()`); PWW_VAE_ATTN=0 / PWW_VAE_TAIL=0 run the
attention as the stock scaled bmm -> fp32 softmax -> bmm sequence / the tail as stock ops. PWW_VAE_TAIL defaults to 1. PWW_VAE_ATTN
defaults to 0: the attention kernel is correct and never stores the scores, but measured slower than the stock sequence at the 64 x 64
latent (profiles/vae_decode.md); PWW_VAE_ATTN=1 turns it on.
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from ._lib import PwwHipError
from .ops import _DT, _ptr, _stream

HEAD_DIM = _lib.VAE_HEAD_DIM
_PARTS = ("group_norm", "conv3x3", "conv_shortcut", "upsample", "attention", "proj_attn", "tail")
_STATS = {k: [0, 0] for k in _PARTS}
_CALLS = [0]


def enabled():
    return os.environ.get("PWW_VAE", "1") != "0"


def attn_enabled():
    """Default OFF: measured at the 64 x 64 latent (N = 4096) pww_vae_attn_fwd takes 261 us against the 122 us of the stock sequence
    (profiles/vae_decode.md), so the stock sequence stays the default and PWW_VAE_ATTN=1 chooses the kernel (no N x N scores in memory)."""
    return os.environ.get("PWW_VAE_ATTN", "0") != "0"


def tail_enabled():
    return os.environ.get("PWW_VAE_TAIL", "1") != "0"


def stats():
    """{part: {"native": n, "stock": n}} since the last reset_stats(), and "decodes": the calls of `decode`. Parts: group_norm (every norm but
    conv_norm_out), conv3x3 (the resnets' convolutions without a shortcut), conv_shortcut (conv2 of the resnets that have one), upsample,
    attention (the mid block's softmax(q k^T) v), proj_attn (its output projection + residual), tail."""
    out = {k: {"native": v[0], "stock": v[1]} for k, v in _STATS.items()}
    out["decodes"] = _CALLS[0]
    return out


def reset_stats():
    for v in _STATS.values():
        v[0] = v[1] = 0
    _CALLS[0] = 0


_ACTIVE = [_STATS]      # the counters `_count` writes to: this module's, or inside `counting(...)` those of the caller (pww_hip.vae_encode)


def _count(part, native):
    _ACTIVE[0][part][0 if native else 1] += 1
    return native


class counting:
    """Inside `with counting(stats):` the helpers below (_group_norm, _conv, _resnet, _attention_block) count into `stats` ({part: [native,
    stock]}) instead of this module's counters: the encoder plug runs on them and keeps counters of its own."""

    def __init__(self, stats):
        self._stats = stats

    def __enter__(self):
        self._prev, _ACTIVE[0] = _ACTIVE[0], self._stats

    def __exit__(self, *exc):
        _ACTIVE[0] = self._prev
        return False


# ---- the structural check ------------------------------------------------------------------------------------------------------------------
def _is_conv(m, k, cin=None, cout=None):
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (k, k) and m.stride == (1, 1) and m.padding == (k // 2, k // 2) and m.dilation == (1, 1)
            and m.groups == 1 and m.padding_mode == "zeros" and m.bias is not None and (cin is None or m.in_channels == cin)
            and (cout is None or m.out_channels == cout))


def _is_norm(m, channels):
    return isinstance(m, nn.GroupNorm) and m.num_channels == channels and m.affine


def _resnet_ok(r):
    c1, c2 = getattr(r, "conv1", None), getattr(r, "conv2", None)
    if not (_is_conv(c1, 3) and _is_conv(c2, 3, c1.out_channels, c1.out_channels) and _is_norm(getattr(r, "norm1", None), c1.in_channels)
            and _is_norm(getattr(r, "norm2", None), c1.out_channels) and getattr(r, "time_emb_proj", None) is None):
        return False
    if getattr(r, "output_scale_factor", 1.0) != 1.0 or getattr(r, "upsample", None) is not None or getattr(r, "downsample", None) is not None:
        return False
    sc = getattr(r, "conv_shortcut", None)
    return sc is None if c1.in_channels == c1.out_channels else _is_conv(sc, 1, c1.in_channels, c1.out_channels)


def _attn_ok(a, channels):
    lins = [getattr(a, n, None) for n in ("query", "key", "value", "proj_attn")]
    return (_is_norm(getattr(a, "group_norm", None), channels) and all(type(m) is nn.Linear and m.bias is not None and m.in_features == channels
                                                                      and m.out_features == channels for m in lins)
            and getattr(a, "num_heads", 1) == 1 and getattr(a, "rescale_output_factor", 1.0) == 1.0)


def covers(vae, require_device=True):
    """True for a float16 / bfloat16 module on a HIP device with the decoder layout of diffusers 0.10.0's AutoencoderKL: post_quant_conv (1 x 1),
    decoder.conv_in, .mid_block (.resnets[0], .attentions[0] -- one head --, .resnets[1]), .up_blocks of ResnetBlock2D without a time embedding
    (+ .upsamplers[0]), .conv_norm_out, .conv_out. sd_standin.TinyVAE, an fp32 module or one on the CPU is not covered.
    require_device=False: the layout and dtype checks alone (what a host without a GPU can ask)."""
    try:
        dec = vae.decoder
        pq, cin, mid = vae.post_quant_conv, dec.conv_in, dec.mid_block
        w = cin.weight
        if not (w.dtype in _DT and (w.is_cuda or not require_device) and _is_conv(pq, 1) and _is_conv(cin, 3, pq.out_channels)):
            return False
        if any(p.dtype != w.dtype or p.device != w.device for m in (pq, dec) for p in m.parameters()):
            return False
        ch = cin.out_channels
        if not (len(mid.resnets) == 2 and len(mid.attentions) == 1 and all(_resnet_ok(r) and r.conv1.in_channels == ch and r.conv1.out_channels == ch
                                                                           for r in mid.resnets) and _attn_ok(mid.attentions[0], ch)):
            return False
        for block in dec.up_blocks:
            if getattr(block, "attentions", None):
                return False
            for r in block.resnets:
                if not (_resnet_ok(r) and r.conv1.in_channels == ch):
                    return False
                ch = r.conv1.out_channels
            ups = getattr(block, "upsamplers", None)
            if ups is not None and not (len(ups) == 1 and _is_conv(getattr(ups[0], "conv", None), 3, ch, ch)):
                return False
        return _is_norm(dec.conv_norm_out, ch) and _is_conv(dec.conv_out, 3, ch)
    except AttributeError:
        return False


# ---- the two kernels of libpww_hip_vae.so --------------------------------------------------------------------------------------------------
def _rows512(t):
    return t.dim() == 3 and t.shape[2] == HEAD_DIM and t.stride(2) == 1 and t.stride(1) % 8 == 0 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0


def attention_takes(q, k, v):
    """True when pww_vae_attn_fwd runs this call: three [B, N, 512] float16 / bfloat16 tensors of one dtype and shape on a HIP device, unit
    stride along the last dim, row and batch strides multiples of 8 elements, 16-byte aligned (slices of one [B, N, 1536] tensor qualify)."""
    return (all(torch.is_tensor(t) and t.is_cuda and t.dtype in _DT and t.dtype == q.dtype and t.shape == q.shape and _rows512(t) for t in (q, k, v))
            and q.shape[0] <= 65535 and q.shape[1] >= 1 and max(t.stride(0) * t.shape[0] for t in (q, k, v)) < 2 ** 31)


def attention(q, k, v, out=None, scale=None):
    """softmax(q k^T / sqrt(512)) v for [B, N, 512] tensors, one head, on pww_vae_attn_fwd: the N x N scores are never stored. `out`: a
    [B, N, 512] tensor with unit stride along the last dim (default: a new dense one)."""
    if not attention_takes(q, k, v):
        raise PwwHipError("vae.attention: needs three [B, N, 512] float16/bfloat16 tensors of one dtype on a HIP device with 16-byte aligned rows")
    B, N, D = q.shape
    if out is None:
        out = torch.empty((B, N, D), dtype=q.dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != q.dtype or not _rows512(out):
        raise PwwHipError("vae.attention: `out` must be a [B, N, 512] tensor of q's dtype with 16-byte aligned rows")
    d = _lib.VaeAttnDesc(ctypes.sizeof(_lib.VaeAttnDesc), _DT[q.dtype], B, N, D, float(scale or 0.0), q.stride(0), q.stride(1), k.stride(0), k.stride(1),
                         v.stride(0), v.stride(1), out.stride(0), out.stride(1))
    lib = _lib.load_vae()
    with torch.cuda.device(q.device):
        _lib.check(lib.pww_vae_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), ctypes.byref(d), _stream()), "pww_vae_attn_fwd", lib)
    return out


def attention_stock(q, k, v):
    """The sequence the kernel replaces: scaled bmm -> fp32 softmax -> bmm, in the storage dtype."""
    probs = torch.softmax((torch.bmm(q, k.transpose(1, 2)) * (q.shape[-1] ** -0.5)).float(), dim=-1).to(q.dtype)
    return torch.bmm(probs, v)


def _tail_desc(x, eps, output):
    B, C, H, W = x.shape
    return _lib.VaeTailDesc(ctypes.sizeof(_lib.VaeTailDesc), _DT[x.dtype], B, H, W, C, _lib.VAE_OUT_UINT8 if output == "uint8" else _lib.VAE_OUT_SAMPLE, float(eps))


def tail_takes(x, norm_weight, norm_bias, weight, bias, groups=32):
    """True when pww_vae_tail_fwd runs this call: a channels_last [B, 128, H, W] float16 / bfloat16 x on a HIP device, 32 groups, an affine of
    its dtype and a [3, 128, 3, 3] weight + [3] bias of its dtype."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _DT and x.shape[1] == _lib.VAE_TAIL_CHANNELS and groups == _lib.VAE_TAIL_GROUPS):
        return False
    return (x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0 and x.numel() < 2 ** 31 and x.shape[0] <= 65535
            and all(torch.is_tensor(t) and t.dtype == x.dtype and t.device == x.device for t in (norm_weight, norm_bias, weight, bias))
            and tuple(norm_weight.shape) == (128,) and tuple(norm_bias.shape) == (128,) and tuple(weight.shape) == (3, 128, 3, 3) and tuple(bias.shape) == (3,))


def tail_moments(x, eps=1e-6):
    """The statistics launch alone: the fp32 [B, chunks, 32, 2] per-chunk (sum, sum of squares) of a channels_last [B, 128, H, W] x, as the
    fused launch reads them. Bitwise repeatable."""
    if not tail_takes(x, x.new_empty(128), x.new_empty(128), x.new_empty(3, 128, 3, 3), x.new_empty(3)):
        raise PwwHipError("vae.tail_moments: needs a channels_last [B, 128, H, W] float16/bfloat16 tensor on a HIP device")
    d = _tail_desc(x, eps, "sample")
    lib = _lib.load_vae()
    nbytes, chunks = int(lib.pww_vae_tail_workspace_bytes(ctypes.byref(d))), int(lib.pww_vae_tail_chunks(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_vae_tail_stats(_ptr(x), None, ctypes.byref(d), _ptr(ws), nbytes, _stream()), "pww_vae_tail_stats", lib)
    return ws[:x.shape[0] * chunks * 64].view(x.shape[0], chunks, 32, 2)


def tail(x, norm_weight, norm_bias, weight, bias, eps=1e-6, output="sample"):
    """conv3x3(silu(group_norm_32(x)), weight) + bias of a channels_last [B, 128, H, W] x, in two launches: output="sample" -> [B, 3, H, W] of
    x's dtype; "uint8" -> the [B, H, W, 3] uint8 image round(255 * clamp(y / 2 + 0.5, 0, 1)), half to even. fp32 from the norm to the output."""
    if output not in ("sample", "uint8"):
        raise PwwHipError("vae.tail: output must be 'sample' or 'uint8'")
    if not tail_takes(x, norm_weight, norm_bias, weight, bias):
        raise PwwHipError("vae.tail: needs a channels_last [B, 128, H, W] float16/bfloat16 x on a HIP device, a [128] affine, a [3, 128, 3, 3] weight "
                          "and a [3] bias of its dtype")
    B, C, H, W = x.shape
    d = _tail_desc(x, eps, output)
    lib = _lib.load_vae()
    nbytes = int(lib.pww_vae_tail_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    out = (torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device) if output == "uint8" else torch.empty((B, 3, H, W), dtype=x.dtype, device=x.device))
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_vae_tail_fwd(_ptr(x), _ptr(norm_weight.contiguous()), _ptr(norm_bias.contiguous()), _ptr(weight.contiguous()), _ptr(bias.contiguous()),
                                        _ptr(out), ctypes.byref(d), _ptr(ws), nbytes, _stream()), "pww_vae_tail_fwd", lib)
    return out


def to_uint8(sample):
    """The stock post-processing of `_pil_from_latents` on the device, in sample's dtype up to the float cast: [B, H, W, 3] uint8."""
    return ((sample / 2 + 0.5).clamp(0, 1).float().permute(0, 2, 3, 1) * 255).round().to(torch.uint8)


def tail_stock(x, norm, conv, output="sample"):
    y = conv(F.silu(F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps)))
    return to_uint8(y) if output == "uint8" else y


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------------
def _norm_takes(x, norm):
    B, C, H, W = x.shape
    return C % 8 == 0 and (H * W) % 8 == 0 and C % norm.num_groups == 0 and norm.num_groups <= 32 and C <= 4096


def _cl(x):
    """A stock op's output back in channels_last (a no-op where it already is), so that the next native op takes it."""
    return x.contiguous(memory_format=torch.channels_last)


def _group_norm(x, norm, act=None):
    if _count("group_norm", _norm_takes(x, norm)):
        return ops.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps, act=act)
    y = F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps)
    return _cl(F.silu(y) if act == "silu" else y)


def _conv(part, x, conv, residual=None, upsample=False):
    if _count(part, ops.conv3x3_takes(x, conv.weight, upsample=upsample)):
        return ops.conv3x3(x, conv.weight, conv.bias, residual=residual, upsample=upsample)
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    y = F.conv2d(x, conv.weight, conv.bias, padding=1)
    return _cl(y if residual is None else residual + y)


def _resnet(r, x):
    h = _conv("conv3x3", _group_norm(x, r.norm1, "silu"), r.conv1)
    h = _group_norm(h, r.norm2, "silu")
    sc = r.conv_shortcut
    if sc is None:
        return _conv("conv3x3", h, r.conv2, residual=x)
    if _count("conv_shortcut", ops.conv3x3_shortcut_takes(h, r.conv2.weight, x, sc.weight) and _lib.load_convtail() is not None):
        return ops.conv3x3_shortcut(h, r.conv2.weight, r.conv2.bias, x, sc.weight, sc.bias)
    return _cl(F.conv2d(x, sc.weight, sc.bias) + F.conv2d(h, r.conv2.weight, r.conv2.bias, padding=1))


def _qkv_weight(a):
    """The [1536, 512] weight and [1536] bias of query | key | value, cached on the module and rebuilt when a parameter was replaced, modified
    in place, moved or cast (as ops._khwc_weight caches on the parameter)."""
    params = [p for m in (a.query, a.key, a.value) for p in (m.weight, m.bias)]
    key = tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in params)
    hit = a.__dict__.get("_pww_qkv")
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    w = torch.cat([a.query.weight.detach(), a.key.weight.detach(), a.value.weight.detach()], 0).contiguous()
    b = torch.cat([a.query.bias.detach(), a.key.bias.detach(), a.value.bias.detach()], 0).contiguous()
    a.__dict__["_pww_qkv"] = (key, w, b)
    return w, b


def _attention_block(a, x):
    """x + proj_attn(attention(group_norm(x))) for a channels_last x: its memory IS the [B, H W, C] rows the GEMMs and the kernel read."""
    B, C, H, W = x.shape
    rows = x.permute(0, 2, 3, 1).reshape(B, H * W, C)              # (a view: x is channels_last)
    t = _group_norm(x, a.group_norm).permute(0, 2, 3, 1).reshape(B, H * W, C)
    w, b = _qkv_weight(a)
    qkv = F.linear(t, w, b)                                        # one stock GEMM: [B, N, 3 C]
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    if _count("attention", attn_enabled() and C == HEAD_DIM and attention_takes(q, k, v)):
        o = attention(q, k, v)
    else:
        o = attention_stock(q, k, v)
    pw, pb = a.proj_attn.weight, a.proj_attn.bias
    if _count("proj_attn", ops.linear_takes(o, pw, bias=pb, residual=rows)):
        y = ops.linear(o, pw, pb, residual=rows)
    else:
        y = F.linear(o, pw, pb) + rows
    return y.reshape(B, H, W, C).permute(0, 3, 1, 2)               # channels_last again


def decode(vae, z, output="sample"):
    """`vae.decode(z).sample` ([B, 3, 8 h, 8 w], the VAE's dtype) or, output="uint8", its [B, 8 h, 8 w, 3] uint8 image, for a VAE `covers()`
    accepts; z: [B, 4, h, w] (already divided by the scaling factor, as for `vae.decode`). Any h, w >= 1."""
    if output not in ("sample", "uint8"):
        raise PwwHipError("vae.decode: output must be 'sample' or 'uint8'")
    if not covers(vae):
        raise PwwHipError("vae.decode: the module has not the AutoencoderKL decoder layout in float16/bfloat16 on a HIP device (pww_hip.vae.covers)")
    _CALLS[0] += 1
    dec = vae.decoder
    with torch.no_grad():
        x = dec.conv_in(vae.post_quant_conv(z.to(dec.conv_in.weight.dtype)))
        x = x.contiguous(memory_format=torch.channels_last)       # once: everything below keeps the format
        mid = dec.mid_block
        x = _resnet(mid.resnets[0], x)
        x = _attention_block(mid.attentions[0], x)
        x = _resnet(mid.resnets[1], x)
        for block in dec.up_blocks:
            for r in block.resnets:
                x = _resnet(r, x)
            if getattr(block, "upsamplers", None) is not None:
                x = _conv("upsample", x, block.upsamplers[0].conv, upsample=True)
        norm, conv = dec.conv_norm_out, dec.conv_out
        x = x.contiguous(memory_format=torch.channels_last)
        if _count("tail", tail_enabled() and tail_takes(x, norm.weight, norm.bias, conv.weight, conv.bias, norm.num_groups)):
            return tail(x, norm.weight, norm.bias, conv.weight, conv.bias, norm.eps, output)
        return tail_stock(x, norm, conv, output)
