"""LoRA adapters on the attention projections, kept UNMERGED and chosen per batch row.

A merged adapter (W + s B A) applies to every row of a UNet call alike. Region prompts evaluate every colour of the map as one more row of
the same call, and the common use of regional prompting is another adapter per region -- so the adapters stay beside the base weights and
every attention projection is followed by  y += s (x A^T) B^T  with A, B and s chosen per row (ops.lora_update: one launch of
libpww_hip_lora.so). The base weights are never touched.

    adapter = load_lora(unet, "style.safetensors", "style")       # or a dict[str, Tensor]
    paint_with_words(..., lora=("style", 0.8), region_loras={(255, 0, 0): "character"})
    unload_lora(unet, "style")

Two key grammars give the same adapter:
    kohya-ss      lora_unet_<module path with "_">.lora_down.weight / .lora_up.weight / .alpha (optional)
    dotted peft   [unet.]<module path>.lora_A.weight / .lora_B.weight (/ .alpha)
The targets are to_q, to_k, to_v and to_out.0 of every CrossAttention module (attn1 and attn2). The effective scale of a row is
scale * alpha / rank (alpha defaults to rank): alpha / rank is folded into B when the factors are stacked, `scale` is the row's.

State. One LoraState per UNet (`state_of`), reachable from every attention module that has a LoRA (`module._pww_lora`: a LoraLayer), because
self-attention never sees the context dict. It holds the row assignment the kernel reads: a device int32 row_adapter[rows] (-1: none) and
an fp32 row_scale[rows], written in place by the sampler per request (per UNet call in eager mode), so a captured hipGraph replays with a
new assignment. Per layer the adapters' factors are stacked into A [n][seg][rank_pad][K] and B [n][seg][N / seg][rank_pad] in the UNet's
dtype, ranks zero-padded to a common multiple of 32 (exact); the stacks are rebuilt on load and unload.
"""
import itertools

import torch

from . import _lib

MAX_ADAPTERS = _lib.LORA_MAX_ADAPTERS
MAX_RANK = _lib.LORA_MAX_RANK
MAX_ROWS = 1024          # rows of one UNet call the assignment arrays hold
TARGETS = ("to_q", "to_k", "to_v", "to_out.0")
_ATTR = "_pww_lora"              # on a CrossAttention module: its LoraLayer
_STATE = "_pww_lora_state"       # on the UNet: its LoraState

_stats = {"kernel": 0, "declined": 0}
_generation = itertools.count(1)     # process-wide: a state that is dropped and made again never repeats a graph signature


def stats():
    """{"kernel": updates that ran on pww_lora_fwd, "declined": updates that ran on the stock-torch formula} since reset_stats()."""
    return dict(_stats)


def reset_stats():
    for k in _stats:
        _stats[k] = 0


class LoraAdapter:
    """One loaded adapter: name, factors {(attention module path, target): (down fp32 [rank, K], up fp32 [N, rank], alpha)}, the keys
    that were ignored (strict=False)."""

    def __init__(self, name, factors, ignored):
        self.name, self.factors, self.ignored = name, factors, tuple(ignored)
        self.rank = max(d.shape[0] for d, _, _ in factors.values())

    def __repr__(self):
        return "LoraAdapter(%r, rank %d, %d projections)" % (self.name, self.rank, len(self.factors))


class LoraLayer:
    """What one attention module carries while any adapter of its UNet touches it: the state and its stacked factors, by projection group."""

    def __init__(self, state, path, module):
        self.state, self.path, self.module = state, path, module
        self._stacks = {}

    def stack(self, names):
        """(A [n][seg][rank_pad][K], B [n][seg][N][rank_pad]) of the projections `names` (e.g. ("to_q", "to_k", "to_v")), one segment each:
        zeros where an adapter lacks a projection, alpha / rank folded into B, built once per (load, group)."""
        ent = self._stacks.get(names)
        if ent is None:
            ent = self._stacks[names] = self.state._build(self, names)
        return ent


def _target_module(attn, target):
    return attn.to_out[0] if target == "to_out.0" else getattr(attn, target)


class LoraState:
    def __init__(self, unet):
        self.adapters = []           # list of LoraAdapter: index = what row_adapter holds
        self.generation = next(_generation)      # renewed on load / unload: captured graphs hold the stacks by address
        self.rank_pad = 0
        self.layers = {}             # attention module path -> LoraLayer
        self.row_adapter = self.row_scale = None
        self._unet = unet

    # -- the row assignment ---------------------------------------------------------------------------------------------------------
    def _device_dtype(self):
        p = next(self._unet.parameters())
        return p.device, p.dtype

    def _ensure_rows(self):
        dev, _ = self._device_dtype()
        if self.row_adapter is None or self.row_adapter.device != dev:
            self.row_adapter = torch.full((MAX_ROWS,), -1, dtype=torch.int32, device=dev)
            self.row_scale = torch.zeros((MAX_ROWS,), dtype=torch.float32, device=dev)
            self.generation = next(_generation)
            for layer in self.layers.values():
                layer._stacks.clear()

    def device_rows(self, adapters, scales):
        """(int32 [R], fp32 [R]) device tensors of one assignment, to hand to `assign` (eager mode prepares one per row class and request)."""
        self._ensure_rows()
        if len(adapters) != len(scales) or len(adapters) > MAX_ROWS:
            raise ValueError("LoRA: %d adapters / %d scales for one call (at most %d rows)" % (len(adapters), len(scales), MAX_ROWS))
        dev = self.row_adapter.device
        return (torch.tensor(list(adapters), dtype=torch.int32).to(dev), torch.tensor(list(scales), dtype=torch.float32).to(dev))

    def assign(self, rows):
        """Write an assignment IN PLACE (the arrays' addresses are what captured launches hold)."""
        a, s = rows
        self.row_adapter[:a.numel()].copy_(a)
        self.row_scale[:s.numel()].copy_(s)

    def signature(self):
        """What a captured graph depends on: None without adapters, else the padded rank and the load generation."""
        return ("lora", self.rank_pad, self.generation) if self.adapters else None

    def index(self, name):
        for i, a in enumerate(self.adapters):
            if a.name == name:
                return i
        raise ValueError("LoRA adapter %r is not loaded (loaded: %s)" % (name, [a.name for a in self.adapters]))

    # -- the stacks -------------------------------------------------------------------------------------------------------------------
    def _rebuild(self):
        for layer in self.layers.values():
            layer.module.__dict__.pop(_ATTR, None)
        self.layers = {}
        self.generation = next(_generation)
        self.rank_pad = max(((a.rank + 31) // 32 * 32 for a in self.adapters), default=0)
        paths = {p for a in self.adapters for p, _ in a.factors}
        mods = dict(self._unet.named_modules())
        for p in sorted(paths):
            layer = LoraLayer(self, p, mods[p])
            self.layers[p] = layer
            mods[p].__dict__[_ATTR] = layer

    def _build(self, layer, names):
        dev, dtype = self._device_dtype()
        mods = [_target_module(layer.module, t) for t in names]
        shapes = {tuple(m.weight.shape[:2]) for m in mods}
        if len(shapes) != 1:
            raise ValueError("LoRA: projections %s of %s do not share one shape (%s)" % (names, layer.path, sorted(shapes)))
        (N, K), n, r = shapes.pop(), len(self.adapters), self.rank_pad
        A = torch.zeros((n, len(names), r, K), dtype=torch.float32)
        B = torch.zeros((n, len(names), N, r), dtype=torch.float32)
        for i, ad in enumerate(self.adapters):
            for g, t in enumerate(names):
                f = ad.factors.get((layer.path, t))
                if f is not None:
                    down, up, alpha = f
                    A[i, g, :down.shape[0]] = down
                    B[i, g, :, :up.shape[1]] = up * (alpha / down.shape[0])
        return A.to(device=dev, dtype=dtype).contiguous(), B.to(device=dev, dtype=dtype).contiguous()


def state_of(unet, create=False):
    """The UNet's LoraState, or None when none was ever loaded (create=False)."""
    st = unet.__dict__.get(_STATE)
    if st is None and create:
        st = unet.__dict__[_STATE] = LoraState(unet)
    return st


def loras(unet):
    """Names of the loaded adapters, in index order."""
    st = state_of(unet)
    return [a.name for a in st.adapters] if st is not None else []


def _attention_paths(unet):
    return [p for p, m in unet.named_modules() if m.__class__.__name__ in ("CrossAttention", "Attention") and hasattr(m, "to_q")]


def _parse(unet, source):
    """-> ({(path, target): {"down" | "up" | "alpha": tensor}}, [foreign keys])."""
    paths = _attention_paths(unet)
    kohya = {"lora_unet_" + (p + "." + t).replace(".", "_"): (p, t) for p in paths for t in TARGETS}
    dotted = {p + "." + t: (p, t) for p in paths for t in TARGETS}
    out, foreign = {}, []
    for key, value in source.items():
        hit = None
        stem, _, suffix = key.partition(".")
        if stem in kohya and suffix in ("lora_down.weight", "lora_up.weight", "alpha"):
            hit = (kohya[stem], {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha"}[suffix])
        else:
            for suffix, what in (("lora_A.weight", "down"), ("lora_B.weight", "up"), ("alpha", "alpha")):
                if key.endswith("." + suffix):
                    stem = key[:-len(suffix) - 1]
                    tgt = dotted.get(stem[5:] if stem.startswith("unet.") else stem)
                    hit = (tgt, what) if tgt is not None else None
                    break
        if hit is None:
            foreign.append(key)
        else:
            out.setdefault(hit[0], {})[hit[1]] = value
    return out, foreign


def load_lora(unet, source, name, strict=True):
    """Load an adapter under `name`: `source` is a dict[str, Tensor] or the path of a .safetensors file. Keys for anything but the
    attention projections raise a ValueError that names them (strict=True) or are listed in `adapter.ignored`; a factor whose shape does
    not fit the UNet always raises. At most 8 adapters per UNet, rank <= 128."""
    if not isinstance(name, str) or not name:
        raise ValueError("LoRA: the adapter's name must be a non-empty string (got %r)" % (name,))
    st = state_of(unet, create=True)
    if name in [a.name for a in st.adapters]:
        raise ValueError("LoRA adapter %r is already loaded" % name)
    if len(st.adapters) >= MAX_ADAPTERS:
        raise ValueError("LoRA: at most %d adapters per UNet (loaded: %s)" % (MAX_ADAPTERS, [a.name for a in st.adapters]))
    if not isinstance(source, dict):
        from safetensors.torch import load_file      # (lazily: only file sources need it)
        source = load_file(str(source))
    parsed, foreign = _parse(unet, source)
    if foreign and strict:
        raise ValueError("LoRA %r: keys outside the attention projections (to_q, to_k, to_v, to_out.0 of attn1 / attn2): %s" % (name, sorted(foreign)))
    if not parsed:
        raise ValueError("LoRA %r: no key names an attention projection of this UNet" % name)
    mods = dict(unet.named_modules())
    factors = {}
    for (path, target), f in sorted(parsed.items()):
        if "down" not in f or "up" not in f:
            raise ValueError("LoRA %r: %s.%s has only %s (both factors are needed)" % (name, path, target, sorted(f)))
        w = _target_module(mods[path], target).weight
        down, up = (t.detach().to("cpu", torch.float32) for t in (f["down"], f["up"]))
        down = down.reshape(down.shape[0], -1) if down.dim() == 4 and tuple(down.shape[2:]) == (1, 1) else down
        up = up.reshape(up.shape[0], -1) if up.dim() == 4 and tuple(up.shape[2:]) == (1, 1) else up
        if down.dim() != 2 or up.dim() != 2 or down.shape[1] != w.shape[1] or up.shape[0] != w.shape[0] or up.shape[1] != down.shape[0]:
            raise ValueError("LoRA %r: %s.%s has factors %s / %s for a weight %s" % (name, path, target, tuple(f["down"].shape), tuple(f["up"].shape),
                                                                                      tuple(w.shape)))
        rank = down.shape[0]
        if not 1 <= rank <= MAX_RANK:
            raise ValueError("LoRA %r: %s.%s has rank %d (at most %d)" % (name, path, target, rank, MAX_RANK))
        alpha = float(f["alpha"]) if "alpha" in f else float(rank)
        factors[(path, target)] = (down, up, alpha)
    adapter = LoraAdapter(name, factors, foreign)
    st.adapters.append(adapter)
    st._rebuild()
    return adapter


def unload_lora(unet, name):
    """Remove the adapter `name`; with the last one gone no attention module keeps an attribute of this module."""
    st = state_of(unet)
    if st is None:
        raise ValueError("LoRA adapter %r is not loaded (loaded: [])" % name)
    del st.adapters[st.index(name)]
    st._rebuild()
    if not st.adapters:
        unet.__dict__.pop(_STATE, None)


# ---- the keywords `lora=` / `region_loras=`: checked without a model, resolved against a UNet, laid out per row -------------------------
def lora_entry(value, what="lora"):
    """`"name"` or `("name", scale)` -> (name, scale), the scale a finite number (default 1.0)."""
    import math
    fields = (value,) if isinstance(value, str) else value
    if not isinstance(fields, (tuple, list)) or not 1 <= len(fields) <= 2 or not isinstance(fields[0], str) or not fields[0]:
        raise ValueError("%s must be an adapter's name or (name, scale) (got %r)" % (what, value))
    scale = fields[1] if len(fields) > 1 else 1.0
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(float(scale)):
        raise ValueError("%s: the scale must be a finite number (got %r)" % (what, scale))
    return fields[0], float(scale)


def row_plan(n, region_colors, lora, region_loras, index):
    """The assignment of one folded call, as Python lists in _fold_regions' order [base x n, region 1 x n, ..., region K x n, uncond x n]
    (without regions: [cond x n, uncond x n]).
      region_colors   per image, the (r, g, b) of its K regions in order (K = 0: [] per image)
      lora            None or (name, scale): every row without an adapter of its own
      region_loras    per image, None or {(r, g, b): (name, scale)}
      index           name -> adapter index (LoraState.index)
    -> (adapters, scales); row `cls * n + j` is image j's row of class cls (0 base, 1 .. K regions, K + 1 unconditional)."""
    K = len(region_colors[0]) if region_colors else 0
    g = (-1, 0.0) if lora is None else (index(lora[0]), lora[1])
    adapters, scales = [], []
    for cls in range(K + 2):
        for j in range(n):
            a, s = g
            if 1 <= cls <= K and region_loras is not None and region_loras[j]:
                own = region_loras[j].get(region_colors[j][cls - 1])
                if own is not None:
                    a, s = index(own[0]), own[1]
            adapters.append(a)
            scales.append(s)
    return adapters, scales
