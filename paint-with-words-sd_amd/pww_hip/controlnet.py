"""ControlNet beside the colour map: a control image (scribble, depth, segmentation ...) steers the geometry while the colour map says which
word goes where.

A ControlNet is the UNet's own down path and mid block, so `install` + `install_blocks` give its encoder every native kernel. What is new per
UNet evaluation are its 1 x 1 "zero convolutions" (thirteen at the SD1.5 topology), the scaling by the conditioning scale and the adds into
the UNet's skip tensors and mid-block output: ONE grouped launch here (ops.control_residuals, libpww_hip_control.so), about 39 small launches
in the stock formulation.

`ControlledUNet` is what the sampler calls in place of the UNet: forward(sample, timestep, encoder_hidden_states).
  * The control image goes through `controlnet_cond_embedding` once per request (`begin_request`), into a static tensor with one row per
    UNet row, [class * n + image]: a row's class (prompt, region prompt, unconditional) does not change the hint, its image does.
  * Each evaluation runs the ControlNet's conv_in + hint, down blocks and mid block. Its cross-attention receives the CONTEXT_TENSOR of the
    UNet's context as a PLAIN tensor: the paint-with-words bias acts in the UNet only. The hidden states are kept; the zero convolutions are
    not called.
  * Native route -- a UNet with the stand-in's top-level layout: its top-level forward is restated, and between the mid block and the up
    blocks sits one grouped launch per ControlNet with the skips given, out of place (the tensors the down path consumed are not written);
    a second ControlNet's launch takes the first's outputs as its skips.
  * Residual route -- any other UNet, or where ops.control_takes declines: one grouped launch without skips per ControlNet (the next net's
    adds into it), or, if the kernel does not take the shapes, the modules times the scale word; the sums go in as
    `down_block_additional_residuals=` / `mid_block_additional_residual=`.
The conditioning scale of every net is a float32 word in device memory that the launch reads when it RUNS, so one captured hipGraph serves
every scale, and a step outside [control_guidance_start, control_guidance_end] replays with the word at 0 (T(skip + 0 x) is the skip bit for
bit); eager and folded mode skip the ControlNet for such a step.

PWW_CONTROL (environment, read per request): "0" the stock sequence (modules, times the scale word, adds), "1" the grouped launch where it
takes the operands, "force" the grouped launch or an error. Default: see DEFAULT below and profiles/control.md. `stats()` / `reset_stats()`.

`covers(net)` decides by layout; diffusers is not installable where this is built, so a diffusers ControlNetModel is covered by layout only
and the tests run on sd_standin.ControlNetModel.
"""
import os
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import PwwHipError

MAX_NETS = 4
# The default of PWW_CONTROL follows the measurement of the grouped launch against the stock sequence it replaces (tools/time_control.py,
# profiles/control.md, section 1): 37.4 us against 201.8 us at the SD1.5 topology, 2 rows, bf16, outside the spread -- on.
DEFAULT = "1"

_STATS = {"evaluations": 0, "skipped_steps": 0, "stock_zero_convs": 0, "declined": 0, "hint_embeddings": 0, "requests": 0}
_REASONS = {}


def mode():
    """PWW_CONTROL: "0" | "1" | "force"."""
    v = os.environ.get("PWW_CONTROL", DEFAULT)
    if v not in ("0", "1", "force"):
        raise ValueError("PWW_CONTROL must be 0, 1 or force (got %r)" % v)
    return v


def stats():
    """Since the last reset_stats(): grouped_launches / grouped_problems (launches of the grouped kernel and the GEMMs they held),
    stock_zero_convs (zero convolutions run as modules), declined (+ decline_reasons: {reason: count}: calls the grouped kernel did not take),
    hint_embeddings (control images embedded: one per net per request), evaluations (UNet evaluations that ran a ControlNet; a hipGraph
    replay counts, its capture does not), skipped_steps (eager / folded evaluations outside the guidance window), requests."""
    out = dict(_STATS)
    out["grouped_launches"], out["grouped_problems"] = ops.CONTROL_LAUNCHES
    out["decline_reasons"] = dict(_REASONS)
    return out


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0
    _REASONS.clear()
    ops.CONTROL_LAUNCHES[0] = ops.CONTROL_LAUNCHES[1] = 0


def _declined(reason):
    _STATS["declined"] += 1
    _REASONS[reason] = _REASONS.get(reason, 0) + 1


# ---- the structural checks -----------------------------------------------------------------------------------------------------------------
def _zero_conv(m):
    return (isinstance(m, nn.Conv2d) and type(m).forward is nn.Conv2d.forward and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0)
            and m.dilation == (1, 1) and m.groups == 1 and m.bias is not None and m.in_channels == m.out_channels)


def covers(net, require_device=True):
    """True for a float16 / bfloat16 module on a HIP device with the ControlNet layout of diffusers >= 0.14: conv_in, time_embedding,
    down_blocks, mid_block, controlnet_cond_embedding (conv_in, blocks, conv_out), controlnet_down_blocks -- plain 1 x 1 nn.Conv2d, at most 15
    --, controlnet_mid_block. require_device=False: the layout and dtype checks alone (what a host without a GPU can ask)."""
    try:
        emb, zeros, mid = net.controlnet_cond_embedding, list(net.controlnet_down_blocks), net.controlnet_mid_block
        ok = (isinstance(net.conv_in, nn.Conv2d) and isinstance(net.down_blocks, nn.ModuleList) and isinstance(net.mid_block, nn.Module)
              and isinstance(net.time_embedding, nn.Module) and isinstance(emb.conv_in, nn.Conv2d) and isinstance(emb.conv_out, nn.Conv2d)
              and all(isinstance(b, nn.Conv2d) for b in emb.blocks) and emb.conv_out.out_channels == net.conv_in.out_channels
              and 1 <= len(zeros) < ops.CONTROL_MAX_PROBLEMS and all(_zero_conv(z) for z in zeros + [mid])
              and zeros[0].in_channels == net.conv_in.out_channels)
        w = net.conv_in.weight
        return bool(ok and w.dtype in (torch.float16, torch.bfloat16) and (w.is_cuda or not require_device))
    except AttributeError:
        return False


def _standin_unet(unet):
    """The stand-in's top-level layout and a forward of the stand-in's class: what the native route restates."""
    fwd = getattr(type(unet), "forward", None)
    return (getattr(fwd, "__module__", "") == "sd_standin.unet" and "forward" not in unet.__dict__
            and all(hasattr(unet, a) for a in ("conv_in", "time_embedding", "down_blocks", "mid_block", "up_blocks", "conv_norm_out", "conv_out", "time_proj_dim")))


# ---- the request ---------------------------------------------------------------------------------------------------------------------------
class ControlRequest:
    """What PwWSampler.sample(control=) takes: nets (1 .. 4 covered ControlNets), images (per net a float tensor [n, 3, H, W] in [0, 1], one
    row per image of the request), scales (one conditioning scale per net), start / end (the guidance window as fractions of the schedule)."""

    def __init__(self, nets, images, scales, start=0.0, end=1.0):
        nets, images, scales = list(nets), list(images), [float(s) for s in scales]
        if not 1 <= len(nets) <= MAX_NETS:
            raise ValueError("controlnet: %d nets (1 .. %d)" % (len(nets), MAX_NETS))
        if len(images) != len(nets) or len(scales) != len(nets):
            raise ValueError("controlnet: %d nets, %d control images, %d conditioning scales" % (len(nets), len(images), len(scales)))
        for net in nets:
            if not covers(net, require_device=False):
                raise ValueError("controlnet: %s has not the ControlNet layout in float16 / bfloat16 (pww_hip.controlnet.covers)" % type(net).__name__)
        for im in images:
            if not (torch.is_tensor(im) and im.dim() == 4 and im.shape[1] == 3 and im.is_floating_point()):
                raise ValueError("controlnet: a control image must be a float tensor [n, 3, H, W]")
        start, end = float(start), float(end)
        if not (0.0 <= start <= 1.0 and 0.0 <= end <= 1.0 and start <= end):
            raise ValueError("controlnet: the guidance window must satisfy 0 <= control_guidance_start <= control_guidance_end <= 1 (got %r, %r)" % (start, end))
        if not all(s == s and abs(s) != float("inf") for s in scales):
            raise ValueError("controlnet: conditioning scales must be finite (got %r)" % (scales,))
        self.nets, self.images, self.scales, self.start, self.end = nets, images, scales, start, end

    def active(self, i, steps):
        """Is step i of `steps` inside the guidance window (diffusers' rule: off while i / steps < start or (i + 1) / steps > end)?"""
        return not (i / steps < self.start or (i + 1) / steps > self.end)

    def words(self, i, steps):
        """The scale word of every net at step i."""
        return self.scales if self.active(i, steps) else [0.0] * len(self.scales)


# ---- the ControlNet's encoder, restated by layout ----------------------------------------------------------------------------------------------
def _time_embedding(model, timestep, sample):
    if not torch.is_tensor(timestep):
        timestep = torch.tensor([timestep], dtype=torch.float32, device=sample.device)
    timestep = timestep.to(sample.device).reshape(-1).expand(sample.shape[0])
    dtype = model.conv_in.weight.dtype
    if isinstance(model.time_embedding, nn.ModuleList):        # the stand-in: two linears around a SiLU
        from sd_standin.unet import timestep_embedding
        temb = timestep_embedding(timestep, model.time_proj_dim).to(dtype)
        return model.time_embedding[1](F.silu(model.time_embedding[0](temb)))
    return model.time_embedding(model.time_proj(timestep).to(dtype))      # diffusers


def _down(blk, x, temb, ctx):
    if hasattr(blk, "has_cross_attention"):                     # diffusers' blocks
        if blk.has_cross_attention:
            return blk(hidden_states=x, temb=temb, encoder_hidden_states=ctx)
        return blk(hidden_states=x, temb=temb)
    return blk(x, temb, ctx)


def _mid(blk, x, temb, ctx):
    if hasattr(blk, "has_cross_attention"):
        return blk(x, temb, encoder_hidden_states=ctx)
    return blk(x, temb, ctx)


def encoder_states(net, sample, timestep, context_tensor, hint):
    """The hidden states the zero convolutions read: conv_in + hint, every output of the down blocks, the mid block's."""
    temb = _time_embedding(net, timestep, sample)
    x = net.conv_in(sample.to(net.conv_in.weight.dtype)) + hint
    hs = [x]
    for blk in net.down_blocks:
        x, outs = _down(blk, x, temb, context_tensor)
        hs.extend(outs)
    hs.append(_mid(net.mid_block, x, temb, context_tensor))
    return hs


def zero_convs(net):
    return list(net.controlnet_down_blocks) + [net.controlnet_mid_block]


def stock_residuals(net, hs, word):
    """The stock formulation: every zero convolution as a module, times the scale (the device word, rounded to the tensors' type)."""
    convs = zero_convs(net)
    _STATS["stock_zero_convs"] += len(convs)
    s = word.to(hs[0].dtype)
    return [conv(h) * s for conv, h in zip(convs, hs)]


class ControlledUNet:
    """The UNet with its ControlNets, called like the UNet. One per (UNet, nets) of a sampler; `begin_request` before the loop, `set_words`
    before every evaluation, `row` = the image of a batch-1 call in eager mode (None: every row)."""

    def __init__(self, unet, nets):
        self.unet, self.nets = unet, list(nets)
        from .attention import install
        for net in self.nets:
            install(net)
        self.words = None            # float32 [MAX_NETS] on the device: net k reads words[k]
        self.hints = [None] * len(self.nets)
        self.row = None
        self.route = None
        self._trace = None           # what the captured forward launched: counted per replay

    @property
    def dtype(self):
        return self.unet.dtype if hasattr(self.unet, "dtype") else next(self.unet.parameters()).dtype

    @property
    def in_channels(self):
        return self.unet.in_channels

    def planned_route(self):
        m = mode()
        return "stock" if m == "0" else ("native" if _standin_unet(self.unet) else "residual") + (":force" if m == "force" else "")

    def signature(self):
        """What a captured graph of this wrapper depends on besides the UNet's own signature: which nets, the hints' shapes, which route."""
        return ("control", tuple(id(n) for n in self.nets), tuple(None if h is None else (tuple(h.shape), h.dtype) for h in self.hints), self.planned_route())

    def begin_request(self, request, n, classes):
        """Embed the request's control images (once per net) into the static hint tensors, rows [class * n + image], and take the route."""
        dev = self.unet.conv_in.weight.device if hasattr(self.unet, "conv_in") else next(self.unet.parameters()).device
        if [id(x) for x in request.nets] != [id(x) for x in self.nets]:
            raise ValueError("controlnet: the request is for other nets than this wrapper")
        if self.words is None or self.words.device != dev:
            self.words = torch.zeros(MAX_NETS, dtype=torch.float32, device=dev)
        for k, (net, image) in enumerate(zip(self.nets, request.images)):
            if not covers(net):
                raise PwwHipError("controlnet: net %d is not a float16 / bfloat16 ControlNet on a HIP device (pww_hip.controlnet.covers)" % k)
            if image.shape[0] != n:
                raise ValueError("controlnet: %d control images for %d images" % (image.shape[0], n))
            w = net.conv_in.weight
            emb = net.controlnet_cond_embedding(image.to(device=w.device, dtype=w.dtype))
            _STATS["hint_embeddings"] += 1
            rows = emb.repeat(classes, 1, 1, 1) if classes > 1 else emb
            if w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last) and not w.is_contiguous():
                rows = rows.contiguous(memory_format=torch.channels_last)
            old = self.hints[k]
            if old is not None and old.shape == rows.shape and old.dtype == rows.dtype and old.device == rows.device:
                old.copy_(rows)         # a captured graph reads the hint by address: same shape (the graph signature), same tensor
            else:
                self.hints[k] = rows.clone(memory_format=torch.preserve_format)
        self.route = self.planned_route()
        self.row = None
        _STATS["requests"] += 1

    def set_words(self, values):
        """The scale words of the evaluation about to run: one asynchronous launch, no host staging buffer (ops.store_f32)."""
        ops.store_f32(self.words, list(values) + [0.0] * (MAX_NETS - len(values)))

    def replayed(self):
        """A captured graph of this wrapper was replayed: the launches it holds ran again."""
        _STATS["evaluations"] += 1
        trace = self._trace
        if trace:
            ops.CONTROL_LAUNCHES[0] += trace[0]
            ops.CONTROL_LAUNCHES[1] += trace[1]
            _STATS["stock_zero_convs"] += trace[2]

    # -- the pieces of one evaluation
    def _states(self, sample, timestep, encoder_hidden_states):
        ctx = encoder_hidden_states
        if ctx is not None and not torch.is_tensor(ctx):
            ctx = ctx["CONTEXT_TENSOR"]                         # the plain tensor: no paint-with-words bias in the ControlNet
        if ctx is not None and ctx.shape[0] == 1 and sample.shape[0] > 1:
            ctx = ctx.expand(sample.shape[0], -1, -1)
        out = []
        for net, hint in zip(self.nets, self.hints):
            h = hint if self.row is None else hint[self.row:self.row + 1]
            if h.shape[0] != sample.shape[0]:
                raise PwwHipError("controlnet: %d rows of hints for a UNet evaluation of %d rows" % (h.shape[0], sample.shape[0]))
            out.append(encoder_states(net, sample, timestep, ctx, h))
        return out

    def _grouped(self, k, hs, skips):
        """Net k's residuals on the grouped kernel -> the outputs, or None where it is not taken (counted, with its reason)."""
        m = mode()
        if m == "0":
            return None
        word, convs = self.words[k:k + 1], zero_convs(self.nets[k])
        why = ops._control_why_not(hs, convs, word, skips)
        if why is None and ops._lib.load_control() is None:
            why = "libpww_hip_control.so is not built"
        if why is not None:
            if m == "force":
                raise PwwHipError("PWW_CONTROL=force: the grouped launch does not take this call: " + why)
            _declined(why)
            return None
        return ops.control_residuals(hs, convs, word, skips=skips)

    def _residuals(self, states, first=0):
        """The residual route's sums over the nets from `first` on: grouped launches without a skip (the next net's adds into the first's), else
        the modules."""
        total = None
        for k in range(first, len(states)):
            hs = states[k]
            got = self._grouped(k, hs, total)
            if got is None:
                res = stock_residuals(self.nets[k], hs, self.words[k:k + 1])
                got = res if total is None else [a + b for a, b in zip(total, res)]
            total = got
        return total

    def forward(self, sample, timestep, encoder_hidden_states=None):
        before = (ops.CONTROL_LAUNCHES[0], ops.CONTROL_LAUNCHES[1], _STATS["stock_zero_convs"])
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        try:
            return self._forward(sample, timestep, encoder_hidden_states)
        finally:
            if capturing:      # a capture runs nothing: its launches are counted when the graph is replayed
                self._trace = (ops.CONTROL_LAUNCHES[0] - before[0], ops.CONTROL_LAUNCHES[1] - before[1], _STATS["stock_zero_convs"] - before[2])
                ops.CONTROL_LAUNCHES[0], ops.CONTROL_LAUNCHES[1], _STATS["stock_zero_convs"] = before
            else:
                _STATS["evaluations"] += 1

    def _forward(self, sample, timestep, encoder_hidden_states):
        unet = self.unet
        states = self._states(sample, timestep, encoder_hidden_states)
        if not self.route.startswith("native"):
            res = self._residuals(states)
            return unet(sample, timestep, encoder_hidden_states=encoder_hidden_states, down_block_additional_residuals=tuple(res[:-1]),
                        mid_block_additional_residual=res[-1])
        # the stand-in's top-level forward, restated: the grouped launches sit between the mid block and the up blocks
        temb = _time_embedding(unet, timestep, sample)
        x = unet.conv_in(sample.to(unet.dtype))
        skips = (x,)
        for blk in unet.down_blocks:
            x, outs = blk(x, temb, encoder_hidden_states)
            skips += outs
        x = unet.mid_block(x, temb, encoder_hidden_states)
        targets, done = list(skips) + [x], 0
        for k, hs in enumerate(states):
            got = self._grouped(k, hs, targets)                 # out of place: the tensors the down path consumed are not written
            if got is None:
                break
            targets, done = got, k + 1
        if done < len(states):                                  # declined: the residual route's arithmetic for the nets that are left
            targets = [t + r for t, r in zip(targets, self._residuals(states, done))]
        skips, x = tuple(targets[:-1]), targets[-1]
        for blk in unet.up_blocks:
            x, skips = blk(x, skips, temb, encoder_hidden_states)
        x = unet.conv_out(F.silu(unet.conv_norm_out(x)))
        return SimpleNamespace(sample=x)

    __call__ = forward
