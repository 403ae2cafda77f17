"""The blocks that CALL the attention path (diffusers==0.10.0 ``ResnetBlock2D`` / ``Transformer2DModel`` /
``UNet2DConditionModel.conv_norm_out``), with their GroupNorm (+ time-embedding addend, + SiLU) on the HIP kernels of ``csrc/pww_norm.hip``.

Installed per INSTANCE (``module.forward = ...``; ``nn.Module.__call__`` and its hooks stay), by class NAME like the reference's own plug
(paint_with_words.py:193-195 selects ``__class__.__name__ == "CrossAttention"``):

* ``ResnetBlock2D`` -- the 0.10.0 forward restated with the two ``norm -> nonlinearity`` pairs and the ``+ temb`` in front of ``norm2`` as ONE op
  each::

      h = conv1(silu(norm1(x)));  h = h + time_emb_proj(silu(temb))[:, :, None, None];  h = conv2(dropout(silu(norm2(h))));
      return (conv_shortcut(x) + h) / output_scale_factor

  and ``time_emb_proj(silu(temb))`` of all blocks as one GEMM per forward (``TembProjections``).
  Blocks this restatement does not cover (``upsample`` / ``downsample`` inside the block, ``time_embedding_norm != "default"``, a nonlinearity
  other than SiLU) keep their own forward.
  The biases of ``conv1`` / ``conv2`` ride along as operands of the next fused op (``pre_bias`` of norm2, ``ops.bias_residual`` for the block's
  output) instead of costing an add launch each. A block that changes its channel count runs ``conv_shortcut(x) + conv2(h)`` as ONE implicit
  GEMM (``ops.conv3x3_shortcut``: the 1 x 1 shortcut as further K-slabs of conv2's kernel) where ``_conv_shortcut_route`` says so.
* ``UpBlock`` (the stand-in) / ``UpBlock2D`` / ``CrossAttnUpBlock2D`` (diffusers 0.10.0) -- the forward restated without
  ``torch.cat([hidden_states, skip], 1)``: each resnet gets the PAIR, and where ``_resnet_cat`` says so its ``norm1`` and its conv2 + shortcut
  read the two tensors where they lie (``ops.group_norm_cat``, ``ops.conv3x3_shortcut_cat``: the same bits as on the concatenated tensor).
  Everything else materialises the concatenation and calls the resnet exactly as the stock block does.
* every other ``nn.GroupNorm`` of the model (``Transformer2DModel.norm``, ``conv_norm_out``) -- the same kernels without addend / activation.
* ``BasicTransformerBlock`` -- ``attn(norm(h)) + h`` and the block's NEXT LayerNorm as one launch (``ops.add_layer_norm``); ``GEGLU`` --
  ``x * gelu(gate)`` as one launch behind its projection; 1 x 1 ``nn.Conv2d`` (``proj_in`` / ``proj_out`` / ``conv_shortcut``) on channels_last
  tensors -- a GEMM over the ``[B H W, C]`` view with the bias in its epilogue.

Inputs the kernels do not take (CPU tensors, fp32, a channel count that is not a multiple of 8 ...) go through the module's ORIGINAL forward:
that is the stock op of the dependency, not a second implementation of this repository. On a GPU without the HIP library ``ops.group_norm``
raises like every other op here.
"""
import os
import types
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

FUSED_NORM = os.environ.get("PWW_FUSED_NORM", "1") != "0"      # A/B switch (bench.py --no-fused-norm sets it)
BATCHED_TEMB = os.environ.get("PWW_BATCHED_TEMB", "1") != "0"  # A/B switch: one time-embedding projection GEMM per forward for all blocks
FOLD_CONV_BIAS = os.environ.get("PWW_FOLD_CONV_BIAS", "1") != "0"      # A/B: conv1 / conv2 biases of a ResnetBlock2D ride in the next fused op
CONV1X1_AS_LINEAR = os.environ.get("PWW_CONV1X1_AS_LINEAR", "1") != "0"  # A/B: 1 x 1 convolutions on channels_last tensors as GEMMs
# A/B: the feed-forward GEMMs with GEGLU / the residual add in their epilogue (csrc/pww_linear.hip) where LINEAR_ROUTES says the HIP call wins.
# "0": never; "force": every shape the kernel takes (tests, tools), whatever the table says
LINEAR = os.environ.get("PWW_LINEAR", "1")
CONV3X3 = os.environ.get("PWW_CONV3X3", "1") != "0"      # A/B: 3 x 3 convolutions on channels_last tensors on the HIP implicit-GEMM kernel
# A/B: the 1 x 1 conv_shortcut of a ResnetBlock2D as further K-slabs of conv2's implicit GEMM (csrc/pww_conv_tail.hip); "0": the 1 x 1 GEMM
# writes its tensor and conv2's epilogue reads it as the residual
CONV_SHORTCUT = os.environ.get("PWW_CONV_SHORTCUT", "1") != "0"
# A/B: the up blocks without `torch.cat([x, skip], 1)`: norm1 and conv2 + shortcut of each of their ResnetBlock2D read the two tensors where they
# lie (csrc/pww_concat.hip); "0": the block's own forward concatenates and the one-source ops run -- the same bits either way
CONCAT = os.environ.get("PWW_CONCAT", "1") != "0"


# ---- what the plug did with the calls it saw (a call the kernels decline must not go unnoticed) ----------------
# per op: [calls taken by the HIP kernels, calls handed to the module's own forward / the stock op]. Counted on the host, i.e. in eager
# passes and while a hipGraph is captured (a replay runs no Python). `stats()` returns a copy, `reset_stats()` zeroes; the first decline of
# a HIP half-precision tensor per (op, reason) also warns once -- under torch.autocast, the reference's own run mode, the whole plug steps
# aside (autocast runs the norms in fp32) and that is worth knowing when a benchmark claims the fused blocks.
_STATS = {k: [0, 0] for k in ("group_norm", "resnet_block", "transformer_block", "geglu", "conv1x1", "conv3x3", "linear", "conv_shortcut", "concat")}
_UNRATED = ("conv1x1", "conv3x3", "linear", "conv_shortcut", "concat")
_warned = set()


def stats():
    """{op: {"fused": n, "declined": n}} since the last reset_stats(), and the hit rate over the norm / elementwise ops (the 1 x 1
    and 3 x 3 convolutions are listed but not rated: an NCHW tensor keeps MIOpen's convolution by the caller's choice of memory format, and
    the UNet's conv_in / conv_out have channel counts the kernel has no tile for; `linear` counts the GEMMs that were offered to the HIP
    linear kernel: "declined" ones run as the stock GEMM by the measured route table; `conv_shortcut` counts the ResnetBlock2D calls that have
    a conv_shortcut: "fused" ones ran it inside conv2's kernel, "declined" ones as the 1 x 1 GEMM in front of conv2; `concat` counts the
    ResnetBlock2D calls of the restated up blocks: "fused" ones read (x, skip) in place, "declined" ones got torch.cat([x, skip], 1))."""
    out = {k: {"fused": v[0], "declined": v[1]} for k, v in _STATS.items()}
    rated = [v for k, v in _STATS.items() if k not in _UNRATED]
    tot = sum(v[0] + v[1] for v in rated)
    out["hit_rate"] = (sum(v[0] for v in rated) / tot) if tot else None
    return out


def reset_stats():
    for v in _STATS.values():
        v[0] = v[1] = 0


def _count(op, fused, x=None, reason=None):
    _STATS[op][0 if fused else 1] += 1
    if not fused and FUSED_NORM and torch.is_tensor(x) and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16):
        key = (op, reason)
        if key not in _warned:
            _warned.add(key)
            warnings.warn("pww_hip.blocks: %s call on a HIP %s tensor handed to the stock op (%s); pww_hip.blocks.stats() counts them"
                          % (op, str(x.dtype).split(".")[-1], reason or "shape / dtype the kernels do not take"), stacklevel=3)


def _why_not(x):
    if torch.is_autocast_enabled():
        return "torch.autocast is on: the norms run in fp32 there"
    if torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad:
        return "autograd is recording: the kernels are forward-only"
    return None


def _takes(x, norm):
    if not (FUSED_NORM and torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float16, torch.bfloat16)):
        return False
    B, C, H, W = x.shape
    w = norm.weight
    return (C % 8 == 0 and (H * W) % 8 == 0 and C % norm.num_groups == 0 and norm.num_groups <= 32 and C <= 4096
            and (w is None or w.dtype == x.dtype) and not torch.is_autocast_enabled()         # (autocast runs group_norm in fp32)
            and not (torch.is_grad_enabled() and (x.requires_grad or (w is not None and w.requires_grad))))


def fused_group_norm(norm, x, add=None, act=None):
    """act(norm(x + add[:, :, None, None])) through the HIP kernels when they take the input, else the same thing from stock ops."""
    if _takes(x, norm) and (add is None or add.dtype == x.dtype):
        return ops.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps, add=add, act=act)
    if add is not None:
        x = x + add[:, :, None, None]
    y = F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps)
    return F.silu(y) if act == "silu" else y


def _group_norm_forward(self, x, *args, **kwargs):
    if args or kwargs or not _takes(x, self):
        _count("group_norm", False, x, "unexpected arguments" if (args or kwargs) else _why_not(x))
        return self._pww_orig_forward(x, *args, **kwargs)
    _count("group_norm", True)
    return fused_group_norm(self, x)


def _is_silu(m):
    return m is None or isinstance(m, nn.SiLU) or m is F.silu


def _resnet_covered(m):
    return (isinstance(getattr(m, "norm1", None), nn.GroupNorm) and isinstance(getattr(m, "norm2", None), nn.GroupNorm)
            and hasattr(m, "conv1") and hasattr(m, "conv2") and getattr(m, "upsample", None) is None and getattr(m, "downsample", None) is None
            and getattr(m, "time_embedding_norm", "default") == "default" and _is_silu(getattr(m, "nonlinearity", None)))


class TembProjections:
    """``time_emb_proj(silu(temb))`` of ALL the plugged ResnetBlock2D of a model as ONE GEMM per forward (22 blocks in the SD1.5 UNet: 22
    SiLU launches on the same [B, 1280] tensor and 22 GEMMs of 2 rows become one each). The concatenated weight is a COPY: it is rebuilt
    when any source parameter was replaced, modified in place (tensor version counter), moved or cast. The result is cached ON the temb
    tensor object (a fresh one every forward; the hit test also compares the tensor's version counter and data pointer), block i takes its
    columns as a view -- `ops.group_norm` reads strided rows."""

    def __init__(self):
        self.linears = []          # (block, offset, width) in registration order
        self.width = 0
        self._sig = None
        self._w = self._b = None

    def register(self, block):
        lin = block.time_emb_proj
        slot = (self, self.width, lin.out_features)
        self.linears.append((lin, self.width, lin.out_features))
        self.width += (lin.out_features + 7) // 8 * 8             # (every block's columns start 16-byte aligned)
        return slot

    def _signature(self, dtype, device):
        sig = [dtype, device]
        for lin, _, _ in self.linears:
            sig.append((lin.weight.data_ptr(), lin.weight._version, lin.weight.dtype))
            sig.append(None if lin.bias is None else (lin.bias.data_ptr(), lin.bias._version))
        return tuple(sig)

    def project(self, temb):
        # the cache entry is valid for THIS tensor in THIS state: a caller that keeps one temb tensor and updates it in place between
        # forwards (static buffers, hipGraph-style input copies) bumps its version counter
        hit = temb.__dict__.get("_pww_temb_proj")
        if hit is not None and hit[0] is self and hit[2] == (temb._version, temb.data_ptr()):
            return hit[1]
        sig = self._signature(temb.dtype, temb.device)
        if sig != self._sig:
            w = torch.zeros(self.width, self.linears[0][0].in_features, dtype=temb.dtype, device=temb.device)
            b = torch.zeros(self.width, dtype=temb.dtype, device=temb.device)
            for lin, off, n in self.linears:
                w[off:off + n] = lin.weight.detach().to(temb.dtype)
                if lin.bias is not None:
                    b[off:off + n] = lin.bias.detach().to(temb.dtype)
            self._w, self._b, self._sig = w, b, sig
        out = F.linear(F.silu(temb), self._w, self._b)
        temb.__dict__["_pww_temb_proj"] = (self, out, (temb._version, temb.data_ptr()))
        return out


def _conv_no_bias(conv, x):
    """`conv(x)` without its bias (the caller hands the bias to the next fused op instead of paying an add launch for it)."""
    return F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)


def _plain_conv(conv):
    return isinstance(conv, nn.Conv2d) and conv.bias is not None and conv.padding_mode == "zeros" and type(conv).forward is nn.Conv2d.forward \
        and "forward" not in conv.__dict__ and not conv._forward_hooks and not conv._forward_pre_hooks


def _resnet_forward(self, *args, **kwargs):
    """diffusers 0.10.0 ``ResnetBlock2D.forward(input_tensor, temb)`` (``up`` / ``down`` = False, ``time_embedding_norm == "default"``). Any other
    call -- later diffusers pass ``scale=`` (0.21 - 0.26: the LoRA scale) -- reaches the module's own forward with its arguments as given."""
    covered = 1 <= len(args) <= 2 and set(kwargs) <= {"temb"} and not (len(args) == 2 and kwargs)
    input_tensor = args[0] if args else None
    if not covered or not _takes(input_tensor, self.norm1):
        _count("resnet_block", False, input_tensor, ("a call beyond (input_tensor, temb): %d positional, keywords %s" % (len(args), sorted(kwargs))) if not covered else _why_not(input_tensor))
        return self._pww_orig_forward(*args, **kwargs)
    temb = args[1] if len(args) == 2 else kwargs.get("temb")
    return _resnet_body(self, input_tensor, temb)


def _resnet_body(self, input_tensor, temb, pair=None):
    """The restated forward behind `_resnet_forward`'s argument checks. pair = (x1, x2): the input is torch.cat([x1, x2], 1), which
    `_resnet_cat` found both of its readers able to take in two parts (input_tensor is None then, and is only made if conv2 + shortcut
    decline after all)."""
    _count("resnet_block", True)
    dtype = pair[0].dtype if pair is not None else input_tensor.dtype
    fold = FOLD_CONV_BIAS and _plain_conv(self.conv1) and _plain_conv(self.conv2) and self.conv1.bias.dtype == dtype
    if pair is not None:
        h = ops.group_norm_cat(pair[0], pair[1], self.norm1.num_groups, self.norm1.weight, self.norm1.bias, self.norm1.eps, act="silu")
    else:
        h = fused_group_norm(self.norm1, input_tensor, act="silu")
    if fold and _conv3x3_route(self.conv1, h):
        h = ops.conv3x3(h, self.conv1.weight)
    else:
        h = _conv_no_bias(self.conv1, h) if fold else self.conv1(h)
    add = None
    if temb is not None and getattr(self, "time_emb_proj", None) is not None:
        slot = self.__dict__.get("_pww_temb_slot")
        if slot is not None and temb.dtype == h.dtype and temb.dim() == 2 and not torch.is_grad_enabled():
            add = slot[0].project(temb)[:, slot[1]:slot[1] + slot[2]]
        else:
            add = self.time_emb_proj(F.silu(temb))
        if add.dtype != h.dtype:
            add = add.to(h.dtype)
    if fold and _takes(h, self.norm2):
        h = ops.group_norm(h, self.norm2.num_groups, self.norm2.weight, self.norm2.bias, self.norm2.eps, add=add, act="silu", pre_bias=self.conv1.bias)
    else:
        if fold:
            h = h + self.conv1.bias[None, :, None, None]
        h = fused_group_norm(self.norm2, h, add=add, act="silu")
    dropout = getattr(self, "dropout", None)
    if dropout is not None:
        h = dropout(h)
    scale = getattr(self, "output_scale_factor", 1.0)
    shortcut = getattr(self, "conv_shortcut", None)
    if pair is not None:
        took = shortcut is not None and _conv_shortcut_route(self, shortcut, h, None, fold, scale, pair=pair)
        _STATS["concat"][0 if took else 1] += 1
        if took:
            return ops.conv3x3_shortcut_cat(h, self.conv2.weight, self.conv2.bias, pair[0], pair[1], shortcut.weight, shortcut.bias)
        input_tensor = torch.cat(pair, dim=1)         # (what `_resnet_cat` could not foresee: the one-source sequence from here on)
        if shortcut is not None:
            _STATS["conv_shortcut"][1] -= 1           # (asked again below)
    if shortcut is not None:
        if _conv_shortcut_route(self, shortcut, h, input_tensor, fold, scale):
            return ops.conv3x3_shortcut(h, self.conv2.weight, self.conv2.bias, input_tensor, shortcut.weight, shortcut.bias)        # conv2 and the shortcut: one GEMM
        input_tensor = shortcut(input_tensor)
    if fold and input_tensor.dtype == h.dtype and input_tensor.shape == (h.shape[0], self.conv2.out_channels) + h.shape[2:] and _conv3x3_route(self.conv2, h):
        out = ops.conv3x3(h, self.conv2.weight, self.conv2.bias, residual=input_tensor)           # input + (conv2(h) + bias): one kernel
    elif fold and input_tensor.dtype == h.dtype and input_tensor.shape[1] % 8 == 0:
        out = ops.bias_residual(input_tensor, _conv_no_bias(self.conv2, h), self.conv2.bias)          # input + (conv2(h) + bias): one launch
    else:
        out = input_tensor + self.conv2(h)
    return out if scale == 1.0 else out / scale


# ---- 3 x 3 convolutions on channels_last tensors: the implicit-GEMM kernel of csrc/pww_conv.hip ----------------------------------------
def _is_conv3x3(m):
    return (isinstance(m, nn.Conv2d) and type(m).forward is nn.Conv2d.forward and m.kernel_size == (3, 3) and m.stride in ((1, 1), (2, 2))
            and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


# Output rows (B Ho Wo) from which MIOpen's own kernel is the faster one for a convolution without a fused upsample: the 64 x 64 and 32 x 32
# levels at batch 8 (16 rows) measured at 0.6 - 0.9x of stock speed on the HIP kernel (profiles/conv3x3_sweep.md); with the upsample fused it wins there too.
STOCK_FROM_ROWS = 16384


def _conv3x3_route(conv, x, upsample=False):
    """Whether this call of the 3 x 3 `conv` runs on the HIP kernel; counts the call either way (not rated: see stats())."""
    ok = (CONV3X3 and FUSED_NORM and torch.is_tensor(x) and x.dim() == 4 and _is_conv3x3(conv) and not torch.is_autocast_enabled() and not (torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad))
          and (conv.bias is None or conv.bias.dtype == x.dtype) and ops.conv3x3_takes(x, conv.weight, conv.stride[0], upsample)
          and (upsample or x.shape[0] * ((x.shape[2] - 1) // conv.stride[0] + 1) * ((x.shape[3] - 1) // conv.stride[0] + 1) < STOCK_FROM_ROWS))
    _STATS["conv3x3"][0 if ok else 1] += 1
    return ok


def _conv_shortcut_route(block, shortcut, h, x, fold, scale, pair=None):
    """Whether `conv_shortcut(x) + conv2(h)` of this ResnetBlock2D call runs as ONE implicit GEMM (ops.conv3x3_shortcut); counts the call
    either way (not rated). It does when the shortcut is a plain 1 x 1 nn.Conv2d with a bias whose forward is its own or this plug's, x is
    a channels_last tensor of the block's dtype, conv2 would take the HIP route with its bias folded, nothing is divided afterwards, and
    the side library is there. A decline leaves today's sequence: the 1 x 1 GEMM, then conv2 with the residual in its epilogue.
    pair = (x1, x2) instead of x: the same question for x = torch.cat([x1, x2], 1) read in two parts (ops.conv3x3_shortcut_cat)."""
    own = shortcut.__dict__.get("forward")
    ok = (CONV_SHORTCUT and fold and scale == 1.0 and _is_conv1x1(shortcut) and shortcut.bias is not None
          and (own is None or getattr(own, "__func__", None) is _conv1x1_forward) and not shortcut._forward_hooks and not shortcut._forward_pre_hooks
          and _is_conv3x3(block.conv2) and block.conv2.stride == (1, 1))
    if ok and pair is not None:
        ok = (all(t.dtype == h.dtype == shortcut.weight.dtype == shortcut.bias.dtype for t in pair)
              and not (torch.is_grad_enabled() and (pair[0].requires_grad or pair[1].requires_grad or shortcut.weight.requires_grad))
              and ops.conv3x3_shortcut_cat_takes(h, block.conv2.weight, pair[0], pair[1], shortcut.weight))
    elif ok:
        ok = (torch.is_tensor(x) and x.dim() == 4 and x.dtype == h.dtype == shortcut.weight.dtype == shortcut.bias.dtype
              and x.is_contiguous(memory_format=torch.channels_last)
              and not (torch.is_grad_enabled() and (x.requires_grad or shortcut.weight.requires_grad))
              and ops.conv3x3_shortcut_takes(h, block.conv2.weight, x, shortcut.weight)
              and ops._lib.load_convtail() is not None)
    if ok:
        ok = _conv3x3_route(block.conv2, h)      # (last: it counts conv2's call under conv3x3, and the declined path asks it again)
        if not ok:
            _STATS["conv3x3"][1] -= 1
    _STATS["conv_shortcut"][0 if ok else 1] += 1
    return ok


def _conv3x3_forward(self, x, *args, **kwargs):
    if not args and not kwargs and _conv3x3_route(self, x):
        return ops.conv3x3(x, self.weight, self.bias, stride=self.stride[0])
    return self._pww_orig_forward(x, *args, **kwargs)


def _upsample_conv(m):
    """The 3 x 3 conv of an ``Upsample2D`` whose forward is nearest-2x interpolate -> conv (diffusers 0.10.0: ``use_conv`` and not
    ``use_conv_transpose``; the conv is ``conv`` or ``Conv2d_0`` by ``name``), else None."""
    if getattr(m, "use_conv_transpose", False) or not getattr(m, "use_conv", True):
        return None
    conv = getattr(m, "Conv2d_0", None) if getattr(m, "name", "conv") != "conv" else getattr(m, "conv", None)
    return conv if _is_conv3x3(conv) and conv.stride == (1, 1) and "forward" not in conv.__dict__ and not conv._forward_hooks and not conv._forward_pre_hooks else None


def _upsample_forward(self, *args, **kwargs):
    """diffusers 0.10.0 ``Upsample2D.forward(hidden_states, output_size=None)`` with the nearest-2x interpolation fused into the conv's gather
    (exact: nearest only copies). An explicit ``output_size``, or anything else, reaches the module's own forward."""
    plain = 1 <= len(args) <= 2 and set(kwargs) <= {"output_size"} and all(a is None for a in list(args[1:]) + list(kwargs.values()))
    x = args[0] if plain and not (len(args) == 2 and kwargs) else None
    conv = _upsample_conv(self)
    if x is not None and conv is not None and x.dim() == 4 and (getattr(self, "channels", None) in (None, x.shape[1])) and _conv3x3_route(conv, x, upsample=True):
        return ops.conv3x3(x, conv.weight, conv.bias, upsample=True)
    return self._pww_orig_forward(*args, **kwargs)


# ---- 1 x 1 convolutions on channels_last tensors are GEMMs over the [B H W, C] view: bias in the GEMM's epilogue, no layout kernels ----
def _conv1x1_forward(self, x, *args, **kwargs):
    if (not args and not kwargs and FUSED_NORM and CONV1X1_AS_LINEAR and torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == self.weight.dtype
            and x.shape[2] * x.shape[3] > 1 and x.is_contiguous(memory_format=torch.channels_last) and not torch.is_autocast_enabled()):
        B, C, H, W = x.shape
        _STATS["conv1x1"][0] += 1
        y = F.linear(x.permute(0, 2, 3, 1).reshape(B * H * W, C), self.weight.reshape(self.out_channels, C), self.bias)
        return y.view(B, H, W, self.out_channels).permute(0, 3, 1, 2)
    _STATS["conv1x1"][1] += 1          # (an NCHW tensor keeps MIOpen's 1 x 1 convolution: a layout choice of the caller, not worth a warning)
    return self._pww_orig_forward(x, *args, **kwargs)


def _is_conv1x1(m):
    return (isinstance(m, nn.Conv2d) and type(m).forward is nn.Conv2d.forward and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0)
            and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


# ---- BasicTransformerBlock / GEGLU -----------------------------------------------------------------------------------------------------
def _ln_takes(x, norm):
    return (FUSED_NORM and torch.is_tensor(x) and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.dim() >= 2
            and len(norm.normalized_shape) == 1 and x.shape[-1] == norm.normalized_shape[0] and x.shape[-1] % 8 == 0 and x.shape[-1] <= 2048
            and (norm.weight is None or norm.weight.dtype == x.dtype) and not torch.is_autocast_enabled()
            and not (torch.is_grad_enabled() and (x.requires_grad or (norm.weight is not None and norm.weight.requires_grad))))


def _transformer_block_covered(m):
    return (all(isinstance(getattr(m, n, None), nn.LayerNorm) for n in ("norm1", "norm2", "norm3")) and hasattr(m, "attn1") and hasattr(m, "attn2")
            and hasattr(m, "ff") and not getattr(m, "only_cross_attention", False))


def _transformer_block_forward(self, *args, **kwargs):
    """diffusers 0.10.0 ``BasicTransformerBlock.forward(hidden_states, context=None, timestep=None)``: ``h = attn1(norm1(h)) + h;
    h = attn2(norm2(h), context) + h; h = ff(norm3(h)) + h`` -- with each residual add and the NEXT norm as one launch. 0.10.0's
    ``Transformer2DModel`` always passes ``timestep=`` (None unless the norms are AdaLayerNorm, which `_transformer_block_covered` excludes):
    a None timestep is accepted and ignored. Every other call -- a real timestep, more positionals, keywords this restatement does not know
    (later diffusers: ``encoder_hidden_states=``, ``attention_mask=``, ``cross_attention_kwargs=`` ...) -- reaches the module's own forward
    with its arguments exactly as they were given."""
    covered = 1 <= len(args) <= 2 and set(kwargs) <= {"context", "timestep"} and kwargs.get("timestep") is None and not (len(args) == 2 and "context" in kwargs)
    hidden_states = args[0] if args else None
    if not covered or not _ln_takes(hidden_states, self.norm1):
        _count("transformer_block", False, hidden_states, ("a call beyond (hidden_states, context, timestep=None): %d positional, keywords %s" % (len(args), sorted(kwargs)))
               if not covered else _why_not(hidden_states))
        return self._pww_orig_forward(*args, **kwargs)
    context = args[1] if len(args) == 2 else kwargs.get("context")
    _count("transformer_block", True)
    h = hidden_states
    n = ops.add_layer_norm(h, self.norm1.weight, self.norm1.bias, self.norm1.eps)
    h, n = ops.add_layer_norm(h, self.norm2.weight, self.norm2.bias, self.norm2.eps, a=self.attn1(n))
    h, n = ops.add_layer_norm(h, self.norm3.weight, self.norm3.bias, self.norm3.eps, a=self.attn2(n, context=context))
    lin = _ff_output_linear(self.ff) if LINEAR != "0" else None
    if lin is not None:
        # `ff(norm3(h)) + h` with the add in the output GEMM's epilogue (no add launch), where the route table takes the shape
        g = self.ff.net[0](n)
        if _linear_route(g, lin.weight, lin.bias, "residual", residual=h):
            return ops.linear(g, lin.weight, lin.bias, residual=h)
        return lin(g) + h
    return self.ff(n) + h


def _ff_output_linear(ff):
    """The output projection of a diffusers FeedForward `net = [GEGLU, Dropout, Linear]` when the block's tail can run as GEGLU -> one GEMM
    with the residual in its epilogue (a dropout that does nothing, a plain biased nn.Linear without hooks), else None."""
    net = getattr(ff, "net", None)
    # the stock class only: a subclass (or a patched class) that brings its own `forward` -- LoRA-scaled, chunked -- keeps it
    if net is None or len(net) != 3 or type(ff).__name__ != "FeedForward" or "forward" in ff.__dict__:
        return None
    owner = next((c for c in type(ff).__mro__ if "forward" in c.__dict__), None)
    if owner is None or owner.__name__ != "FeedForward":
        return None
    act, drop, lin = net[0], net[1], net[2]
    if act.__class__.__name__ != "GEGLU" or not isinstance(drop, nn.Dropout) or (drop.training and drop.p > 0):
        return None
    if type(lin) is not nn.Linear or lin.bias is None or lin._forward_hooks or lin._forward_pre_hooks or "forward" in lin.__dict__ or ff._forward_hooks or ff._forward_pre_hooks:
        return None
    return lin


# (rows M, K, N, epilogue) of the SD1.5 UNet at 2 rows on which ops.linear measured faster than the stock sequence (hipBLASLt GEMM + pww_geglu, or
# GEMM + add), replayed from a hipGraph on MI355X: tools/time_linear.py --sweep, profiles/linear_sweep.md. Everything else -- shapes outside
# the table, shapes the stock route wins, the large M of the batch-8 configs -- keeps the stock GEMM.
LINEAR_ROUTES = frozenset([
    (8192, 320, 2560, "geglu"),        # 41.6 us against 51.5 (GEMM 35.0 + pww_geglu)
    (2048, 640, 5120, "geglu"),        # 25.7 against 32.8
    (512, 1280, 10240, "geglu"),       # 25.6 against 27.7
    (128, 1280, 10240, "geglu"),       # 14.1 against 18.3
    (512, 5120, 1280, "residual"),     # 21.5 against 24.4 (GEMM 21.8 + add); the output linears of the other levels lose: 26.1 / 19.1, 22.8 / 19.4, 14.0 / 13.4
])


def _linear_route(x, weight, bias, epilogue, residual=None):
    """Whether this GEMM (x [..., K], weight [N, K], epilogue "geglu" / "residual") runs on the HIP linear kernel; counts the call either way
    (not rated: see stats()). Operands the library would refuse (a misaligned bias, a residual whose rows have no common pitch of a multiple of
    8 elements) decline to the stock GEMM like a shape outside the table. The table is keyed by shape alone, not by dtype: it was measured in
    bf16, and an fp16 run of the same shapes takes the same routes without a timing of its own."""
    ok = (LINEAR != "0" and FUSED_NORM and not torch.is_autocast_enabled() and torch.is_tensor(x) and bias is not None and bias.dtype == x.dtype
          and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)) and ops.linear_takes(x, weight, epilogue == "geglu", bias=bias, residual=residual)
          and (LINEAR == "force" or (x.numel() // x.shape[-1], x.shape[-1], weight.shape[0], epilogue) in LINEAR_ROUTES))
    _STATS["linear"][0 if ok else 1] += 1
    return ok


def _plain_linear(lin):
    return type(lin) is nn.Linear and lin.bias is not None and not lin._forward_hooks and not lin._forward_pre_hooks and "forward" not in lin.__dict__


def _geglu_forward(self, x, *args, **kwargs):
    """diffusers ``GEGLU.forward(hidden_states)``; later versions add ``scale`` (0.21 - 0.26): anything extra -> the module's own forward."""
    if args or kwargs:
        _count("geglu", False, x, "arguments beyond (hidden_states): %s" % (sorted(kwargs) or len(args)))
        return self._pww_orig_forward(x, *args, **kwargs)
    if _plain_linear(self.proj) and _linear_route(x, self.proj.weight, self.proj.bias, "geglu"):
        _count("geglu", True)
        return ops.linear(x, self.proj.weight, self.proj.bias, geglu=True)          # projection and GEGLU: one kernel
    h = self.proj(x)
    if FUSED_NORM and h.is_cuda and h.dtype in (torch.float16, torch.bfloat16) and h.shape[-1] % 16 == 0 and not torch.is_autocast_enabled() \
            and not (torch.is_grad_enabled() and h.requires_grad):
        _count("geglu", True)
        return ops.geglu(h)
    _count("geglu", False, h, _why_not(h))
    a, gate = h.chunk(2, dim=-1)
    return a * F.gelu(gate)


# ---- the up blocks without torch.cat([x, skip], 1) -----------------------------------------------------------------------------------------
# class name -> the parameters of its forward, in order: the stand-in's UpBlock, diffusers 0.10.0's UpBlock2D and CrossAttnUpBlock2D
_UP_BLOCKS = {
    "UpBlock": ("x", "skips", "temb", "ctx"),
    "UpBlock2D": ("hidden_states", "res_hidden_states_tuple", "temb", "upsample_size"),
    "CrossAttnUpBlock2D": ("hidden_states", "res_hidden_states_tuple", "temb", "encoder_hidden_states", "upsample_size"),
}


def _no_hooks(m):
    return not m._forward_hooks and not m._forward_pre_hooks and not nn.modules.module._global_forward_hooks and not nn.modules.module._global_forward_pre_hooks


def _resnet_cat(res, x1, x2, temb):
    """`res(torch.cat([x1, x2], 1), temb)` of an up block. Where the block is plug-covered and BOTH readers of the concatenation take it in
    two parts -- norm1 (ops.group_norm_cat) and conv2 + shortcut (ops.conv3x3_shortcut_cat, asked inside the body once conv2's input
    exists) -- the tensor is never made; every other case materialises it and calls the block exactly as the stock up block does.
    Counted under `concat` either way (not rated)."""
    own = res.__dict__.get("forward")
    shortcut = getattr(res, "conv_shortcut", None)
    ok = (CONCAT and CONV_SHORTCUT and FUSED_NORM and getattr(own, "__func__", None) is _resnet_forward and _no_hooks(res)
          and torch.is_tensor(x1) and torch.is_tensor(x2) and x1.dtype == x2.dtype and not torch.is_autocast_enabled()
          and not (torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad))
          and (temb is None or torch.is_tensor(temb))
          and shortcut is not None and _is_conv1x1(shortcut) and shortcut.bias is not None and getattr(res, "output_scale_factor", 1.0) == 1.0
          and x1.dim() == 4 and x2.dim() == 4 and x1.shape[1] % 64 == 0 and x2.shape[1] % 64 == 0
          and x1.shape[1] + x2.shape[1] == res.norm1.num_channels == shortcut.in_channels
          and res.norm1.weight is not None and res.norm1.weight.dtype == x1.dtype
          and not (torch.is_grad_enabled() and res.norm1.weight.requires_grad)
          and FOLD_CONV_BIAS and _plain_conv(res.conv1) and _plain_conv(res.conv2) and res.conv1.bias.dtype == x1.dtype
          and _is_conv3x3(res.conv2) and res.conv2.stride == (1, 1) and res.conv2.weight.dtype == x1.dtype
          and res.conv2.in_channels % 64 == 0 and res.conv2.out_channels % 64 == 0
          and x1.shape[0] * x1.shape[2] * x1.shape[3] < STOCK_FROM_ROWS
          and ops.group_norm_cat_takes(x1, x2, res.norm1.num_groups, res.norm1.weight, res.norm1.bias))
    if ok:
        return _resnet_body(res, None, temb, pair=(x1, x2))
    _STATS["concat"][1] += 1
    return res(torch.cat([x1, x2], dim=1), temb)


def _up_block_covered(m):
    res, att, ups = getattr(m, "resnets", None), getattr(m, "attentions", None), getattr(m, "upsamplers", None)
    return (m.__class__.__name__ in _UP_BLOCKS and isinstance(res, nn.ModuleList) and len(res) > 0
            and (att is None or (isinstance(att, nn.ModuleList) and len(att) == len(res))) and (ups is None or isinstance(ups, nn.ModuleList))
            and (m.__class__.__name__ != "CrossAttnUpBlock2D" or att is not None))


def _up_block_forward(self, *args, **kwargs):
    """The forward of an up block restated without the concatenation: the stand-in's ``UpBlock.forward(x, skips, temb, ctx)`` and diffusers
    0.10.0's ``UpBlock2D.forward(hidden_states, res_hidden_states_tuple, temb=None, upsample_size=None)`` /
    ``CrossAttnUpBlock2D.forward(hidden_states, res_hidden_states_tuple, temb=None, encoder_hidden_states=None, upsample_size=None)``::

        for resnet (, attn): hidden = resnet(cat([hidden, skips.pop()], 1), temb) (; hidden = attn(hidden, context)); upsamplers; return

    with each ``resnet(cat(...))`` handed to `_resnet_cat` as the pair. Any call this restatement does not know (other keywords, more
    positionals, gradient checkpointing while training, hooks on the block, fewer skips than resnets), and every call with PWW_CONCAT=0,
    reaches the module's own forward with its arguments untouched."""
    names = _UP_BLOCKS[self.__class__.__name__]
    standin = self.__class__.__name__ == "UpBlock"
    vals = dict(zip(names, args))
    known = CONCAT and len(args) <= len(names) and all(k in names and k not in vals for k in kwargs) and _no_hooks(self)
    if known:
        vals.update(kwargs)
        skips = vals.get(names[1])
        known = (names[0] in vals and isinstance(skips, (tuple, list)) and len(skips) >= len(self.resnets) and (not standin or len(vals) == len(names))
                 and not (self.training and getattr(self, "gradient_checkpointing", False)))
    if not known:
        return self._pww_orig_forward(*args, **kwargs)
    x, temb = vals[names[0]], vals.get("temb")
    attentions, upsamplers = getattr(self, "attentions", None), getattr(self, "upsamplers", None)
    for i, res in enumerate(self.resnets):
        x = _resnet_cat(res, x, skips[-1], temb)
        skips = skips[:-1]
        if attentions is not None:
            x = attentions[i](x, vals["ctx"]) if standin else attentions[i](x, encoder_hidden_states=vals.get("encoder_hidden_states")).sample
    if upsamplers is not None:
        if standin:
            x = upsamplers[0](x)
        else:
            for up in upsamplers:
                x = up(x, vals.get("upsample_size"))
    return (x, skips) if standin else x


def install_blocks(unet):
    """Put the fused norms under every ``ResnetBlock2D`` and every other ``nn.GroupNorm`` of `unet`. Returns (resnets, norms) patched."""
    n_res = n_gn = 0
    owned = set()
    plans = {}                 # time-embedding width -> one batched projection for all blocks that share it
    for m in unet.modules():
        if m.__class__.__name__ == "ResnetBlock2D" and _resnet_covered(m):
            if "_pww_orig_forward" not in m.__dict__:
                m.__dict__["_pww_orig_forward"] = m.forward
                m.forward = types.MethodType(_resnet_forward, m)
                lin = getattr(m, "time_emb_proj", None)
                if BATCHED_TEMB and isinstance(lin, nn.Linear):
                    m.__dict__["_pww_temb_slot"] = plans.setdefault(lin.in_features, TembProjections()).register(m)
            owned.update((id(m.norm1), id(m.norm2), id(m.conv1), id(m.conv2)))
            n_res += 1
    for m in unet.modules():
        name, fwd = m.__class__.__name__, None
        if isinstance(m, nn.GroupNorm) and id(m) not in owned:
            fwd = _group_norm_forward
            n_gn += 1
        elif name == "BasicTransformerBlock" and _transformer_block_covered(m):
            fwd = _transformer_block_forward
        elif name == "GEGLU" and isinstance(getattr(m, "proj", None), nn.Linear):
            fwd = _geglu_forward
        elif _is_conv1x1(m):
            fwd = _conv1x1_forward
        elif name == "Upsample2D" and _upsample_conv(m) is not None:
            fwd = _upsample_forward
            owned.add(id(_upsample_conv(m)))
        elif _is_conv3x3(m) and id(m) not in owned:
            fwd = _conv3x3_forward
        elif name in _UP_BLOCKS and _up_block_covered(m):
            fwd = _up_block_forward
        if fwd is not None and "_pww_orig_forward" not in m.__dict__:
            m.__dict__["_pww_orig_forward"] = m.forward
            m.forward = types.MethodType(fwd, m)
    return n_res, n_gn


def uninstall_blocks(unet):
    for m in unet.modules():
        if "_pww_orig_forward" in m.__dict__:
            del m.__dict__["_pww_orig_forward"]
            m.__dict__.pop("forward", None)
            m.__dict__.pop("_pww_temb_slot", None)
