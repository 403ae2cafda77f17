"""The Paint-with-Words attention plug for PyTorch-ROCm, backed by libpww_hip.so.

Mirrors the reference's interface for this path (paint_with_words/paint_with_words.py, cited per
function): ``inj_forward`` has the same signature and context protocol as the reference's
(:60-125) and is installed by the same class-level patch (:193-195); ``PwWAttnProcessor`` offers the
same computation through the attention-processor plug point of newer diffusers.

What changes is WHERE the arithmetic happens: projections stay torch ``nn.Linear`` (hipBLASLt), the
head split / merge disappears into kernel strides, and scores + bias + softmax + PV run in one fused
HIP kernel. The user's ``weight_function(w, sigma, qk)`` still receives ``qk`` -- as a ``QKProxy``
whose reductions are computed by the score-reduction kernel instead of from a materialised tensor.
"""
import collections
import math
import os
import warnings

import torch
import torch.nn.functional as F

from . import ops
from ._lib import PwwHipError

_HALF = (torch.float16, torch.bfloat16)
ROW_GATE = "_PWW_ROW_GATE"   # private context key: fp32 [B] per-row bias coefficient (see pww_hip/sampler.py)
_LAZY_W = True               # hand weight_function a ScaledW instead of the raw map (see ScaledW)
KV_CACHE = "_PWW_KV_CACHE"   # private context key: {id(attn): (attn, [B, 77, 2C] fused K|V projection)} for one request
COEFF_SLOTS = "_PWW_COEFF_SLOTS"   # private context key: CoeffSlots (hipGraph mode: the weight function's per-step scalars live in device words)
BIAS_COLS = "_PWW_BIAS_COLS"       # private context key: int, columns >= this of every weight map of the context are zero
COMPACT_W = "_PWW_COMPACT_W_"      # private context key prefix: compact form [N, R] (or [B, N, R]) of CROSS_ATTENTION_WEIGHT_<N>
COMPACT_IDX = "_PWW_COMPACT_IDX"   # private context key: int32 [R] (or [B, R]) columns of the compact slots, -1 = unused
GATED_ROWS = "_PWW_GATED_ROWS"     # private context key: int, the kernels' work-distribution hint: _PWW_ROW_GATE is non-zero for exactly the first so many rows, 0 after (a CFG-folded batch); 0 = no such split, every row may be biased (negative regions)
COND_ROWS = "_PWW_COND_ROWS"       # private context key: int, the first so many rows are the conditional ones -- what the attention-map recorder records. Only present when it differs from _PWW_GATED_ROWS (negative regions: the unconditional rows are biased too)
ATTN_RECORDER = "_PWW_ATTN_RECORDER"   # private context key of CONDITIONAL dicts: attnmaps.AttentionRecorder (pww_hip.record_attention_maps); absent = nothing is recorded
# Where the score statistic of `weight_function(w, sigma, qk)` is formed (round 5): ALWAYS outside the attention launch -- as partials
# that the attention launch folds at entry (pww_cross_attn_fwd_parts: nothing waits for another workgroup, nothing has to be resident,
# no time-out path) -- either in the epilogue of the to_q GEMM (pww_qproj_stat, where qproj_route says it wins) or by one small launch
# over the finished Q of the stock GEMM (pww_qk_parts: the C = 1280 layers). PWW_FUSED_CROSS=1 selects round 3's form instead (statistic
# + device-scope hand-off inside the attention launch, pww_cross_attn_fwd_fused: needs every workgroup resident at once): TEST / A-B only,
# and since round 6 only with libpww_hip_experiments.so built (the product library does not hold that launch).
FUSED_CROSS = os.environ.get("PWW_FUSED_CROSS", "0") == "1"
# the C = 320 cross-attention layers with to_out (+ bias) applied INSIDE the attention launch
# (pww_cross_attn_fwd_parts_out: one workgroup per 128 query rows walks all heads, then multiplies its O image with W_o). Built, pinned
# to the two-launch route bit for bit on the test shapes, and measured: 34 us against 18 us (small kernel + the stock GEMM with its bias
# epilogue) at the 2 folded rows of a batch-1 request, 38 against 41 at 8 rows, 71 against 73 at 16 (profiles/r05_to_out_epilogue.md) --
# heads run one after the other inside a workgroup where the two-launch route runs them on eight CUs. Round 6: NOT a product route any
# more (no environment switch); the kernel lives in libpww_hip_experiments.so and the tests / tools set this flag themselves.
FUSE_TO_OUT = False
# Per-head / per-row score statistics (qk.amax(dim=(1, 2), keepdim=True), qk.std(dim=-1, keepdim=True), ...) on the launches of
# libpww_hip_scope.so: default on; PWW_SCOPED_STATS=0 keeps such weight functions on the materialised route (Q K^T as a tensor, a dense
# [B * heads, N, M] bias) -- tests and tools/time_scoped_stats.py compare the two routes in one process by setting this flag.
SCOPED_STATS = os.environ.get("PWW_SCOPED_STATS", "1") != "0"
SCOPE_IMAGE, SCOPE_HEAD, SCOPE_ROW = 0, ops.SCOPE_HEAD, ops.SCOPE_ROW      # what a LazyStat reduces over: all of an image's scores / one head's / one query row's
QPROJ_STAT = os.environ.get("PWW_QPROJ_STAT", "1")       # "1" where it wins (default) | "0" never | "all" wherever the kernel supports the shape
# LoRA adapters (pww_hip/lora.py): a module that any loaded adapter touches carries a lora.LoraLayer under this attribute, and every one of
# its projections is followed by ops.lora_update -- the low-rank update with the adapter and scale of each batch row. Such a layer declines
# the to_q-GEMM-with-statistic route (the statistic would be formed over an un-adapted Q) and the opt-in attention + to_out launch; the
# decision is per layer and static while an adapter is loaded. Without the attribute none of these branches is entered.
LORA_ATTR = "_pww_lora"
_Q, _KV, _QKV, _OUT = ("to_q",), ("to_k", "to_v"), ("to_q", "to_k", "to_v"), ("to_out.0",)


def _lora_update(lo, y, x, names):
    """y += s (x A^T) B^T per row for the projections `names` of the layer (one column segment each), in place."""
    return ops.lora_update(y, x, lo.stack(names), lo.state, len(names))


def qproj_route(C, D):
    """Does `to_q` + statistic as ONE launch beat stock GEMM + the round-3 fused launch for a layer of C channels and head dim D?
    Per-shape measurement, both routes back to back on MI355X (profiles/r04_qproj.md): the projection kernel's tile is a whole number of
    heads in 160 channels, so it keeps up with hipBLASLt for C = 320 (every head dim) and for C = 640 when 160 % D == 0 (SD1.5: +5 us on the
    GEMM, -8 on the attention); wider layers meet too few workgroups and a long contraction (C = 1280: tie at 2 rows x 256 tokens, -4 us at
    64 tokens), SD2.1's C = 640 / d = 64 needs 320-channel tiles (+10 us on the GEMM)."""
    if QPROJ_STAT == "all":
        return True
    return QPROJ_STAT != "0" and (C <= 320 or (C <= 640 and 160 % D == 0))
_warned = set()


def _warn_once(key, msg):
    if key not in _warned:
        _warned.add(key)
        warnings.warn(msg, stacklevel=3)


class LazyStat:
    """``scale * reduce(qk)`` as handed back by QKProxy.max() / .min() / .mean() / .std() / .abs().max().

    All the shipped weight functions only ever MULTIPLY this by Python numbers and by the weight map, so the value is
    kept symbolic: (statistics tensor of pww_qk_reduce, which statistic, Python scale). If it reaches the kernel that
    way (through ScaledW), the kernel forms the coefficient itself (pww_cross_attn_fwd_stat) and the three or four
    [B]-sized elementwise launches per cross-attention layer and step disappear. Any other use -- arithmetic with
    tensors, torch functions, .item(), comparison ... -- materialises the [B,1,1,1] / 0-dim fp32 tensor the old path
    produced and carries on with it, unchanged.

    scope: SCOPE_IMAGE (the global reductions above), SCOPE_HEAD (`qk.amax(dim=(1, 2), keepdim=True)` ...: stands for a [B*heads, 1, 1]
    tensor) or SCOPE_ROW (`qk.std(dim=-1, keepdim=True)` ...: [B*heads, N, 1]). A scoped statistic remembers the call it came from and
    materialises by making that very call on the materialised scores."""
    __slots__ = ("_proxy", "kind", "scale", "_t", "scope", "_call")

    def __init__(self, proxy, kind, scale=1.0, scope=SCOPE_IMAGE, call=None):
        self._proxy, self.kind, self.scale, self._t = proxy, kind, scale, None
        self.scope, self._call = scope, call        # call = (method name, args, kwargs, on qk.abs()?) of a scoped reduction

    def stats(self):
        return self._proxy._st()

    def materialize(self):
        if self._t is None and self.scope != SCOPE_IMAGE:
            name, args, kw, absolute = self._call
            full = self._proxy._materialize()
            t = getattr(full.abs() if absolute else full, name)(*args, **kw)
            self._t = t if self.scale == 1.0 else t * self.scale
        if self._t is None:
            st, n = self._proxy._st(), self._proxy._count()
            if self.kind == ops.STAT_MAX:
                t = st[:, 0]
            elif self.kind == ops.STAT_MIN:
                t = st[:, 1]
            elif self.kind == ops.STAT_MEAN:
                t = st[:, 2] / n
            elif self.kind == ops.STAT_ABSMAX:
                t = torch.maximum(st[:, 0].abs(), st[:, 1].abs())
            else:   # STAT_STD: unbiased, like torch.std
                t = ((st[:, 3] - st[:, 2] * st[:, 2] / n) / max(n - 1, 1)).clamp_min(0)
            t = self._proxy._shape_out(t)
            if self.kind == ops.STAT_STD:
                t = t.sqrt()
            self._t = t if self.scale == 1.0 else t * self.scale
        return self._t

    def _times(self, other, divide=False):
        if isinstance(other, (int, float)) and not isinstance(other, bool):
            return LazyStat(self._proxy, self.kind, self.scale / other if divide else self.scale * other, self.scope, self._call)
        return None

    def __mul__(self, other):
        r = self._times(other)
        if r is not None:
            return r
        if isinstance(other, ScaledW):
            return other * self
        return self.materialize() * other

    __rmul__ = __mul__

    def __truediv__(self, other):
        r = self._times(other, divide=True)
        return r if r is not None else self.materialize() / other

    def __neg__(self):
        return LazyStat(self._proxy, self.kind, -self.scale, self.scope, self._call)

    def __rtruediv__(self, other): return other / self.materialize()
    def __add__(self, other): return self.materialize() + other
    def __radd__(self, other): return other + self.materialize()
    def __sub__(self, other): return self.materialize() - other
    def __rsub__(self, other): return other - self.materialize()
    def __pow__(self, other): return self.materialize() ** other
    def __float__(self): return float(self.materialize())
    def __bool__(self): return bool(self.materialize())
    def __lt__(self, other): return self.materialize() < other
    def __le__(self, other): return self.materialize() <= other
    def __gt__(self, other): return self.materialize() > other
    def __ge__(self, other): return self.materialize() >= other
    def __getitem__(self, idx): return self.materialize()[idx]

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        conv = lambda a: a.materialize() if isinstance(a, LazyStat) else a  # noqa: E731
        return func(*[conv(a) for a in args], **{k: conv(v) for k, v in (kwargs or {}).items()})


def _reduction_scope(name, args, kw):
    """SCOPE_HEAD / SCOPE_ROW if `qk.<name>(*args, **kw)` is one of the scoped reductions that stay symbolic -- dim = (1, 2) / (-2, -1)
    (tuple or list, either order) or dim = 2 / -1, positional or by name, keepdim=True, for std the torch default (unbiased) -- else None."""
    if any(k not in ("dim", "keepdim", "unbiased") for k in kw) or ("unbiased" in kw and (name != "std" or kw["unbiased"] is not True)):
        return None
    if len(args) > (1 if name == "std" else 2) or (args and "dim" in kw) or (len(args) == 2 and "keepdim" in kw):
        return None
    dim = args[0] if args else kw.get("dim")
    keepdim = args[1] if len(args) == 2 else kw.get("keepdim", False)
    if keepdim is not True:
        return None
    is_int = lambda x: isinstance(x, int) and not isinstance(x, bool)  # noqa: E731
    if is_int(dim):
        return SCOPE_ROW if dim in (2, -1) else None
    if isinstance(dim, (tuple, list)) and len(dim) == 2 and all(is_int(x) and -3 <= x < 3 for x in dim):
        return SCOPE_HEAD if sorted(x % 3 for x in dim) == [1, 2] else None
    return None


class QKProxy:
    """Stands in for the raw score tensor ``qk = Q K^T`` ([B*heads, N, M]) that the reference hands
    to ``weight_function`` (:87, :106). Global reductions -- all the shipped weight functions use
    (``qk.max()`` :402-405 / runner.py:104, ``qk.std()`` README.md:152) -- are answered by
    ``pww_qk_reduce`` without materialising the tensor. Anything else materialises ``qk`` with a
    plain batched GEMM (correct, slower) and delegates to the real tensor.

    With batch > 1 the reductions are PER IMAGE (the reference only ever sees batch 1): they return
    a [B, 1, 1, 1] tensor so the resulting bias broadcasts to [B, heads, N, M].
    """

    def __init__(self, q, k, heads):
        """q: the [B, N, C] query tensor, or a _LazyQuery (cross-attention: the projection itself is deferred -- when the weight
        function only asks for a global reduction, Q and the statistic come out of ONE launch, ops.qproj_stat)."""
        self._q_src, self._k, self._heads = q, k, heads
        self._stats = None
        self._full = None
        B, N, C = q.shape
        self.shape = torch.Size((B * heads, N, k.shape[1]))
        self.dtype = q.dtype
        self.device = q.device

    @property
    def _q(self):
        src = self._q_src
        return src.get() if isinstance(src, _LazyQuery) else src

    # -- lazily computed per-image statistics ---------------------------------------------------
    def _st(self):
        if self._stats is None:
            self._stats = ops.qk_stats(self._q, self._k, self._heads)  # [B, 4] float64
        return self._stats

    def _count(self):
        return self.shape[0] // self._q_src.shape[0] * self.shape[1] * self.shape[2]

    def _shape_out(self, t):
        t = t.to(torch.float32)
        return t.reshape(()) if t.numel() == 1 else t.reshape(-1, 1, 1, 1)

    def max(self, *args, **kw):
        if args or kw:
            return self._materialize().max(*args, **kw)
        return LazyStat(self, ops.STAT_MAX)

    def min(self, *args, **kw):
        if args or kw:
            return self._materialize().min(*args, **kw)
        return LazyStat(self, ops.STAT_MIN)

    def _scoped(self, kind, name, args, kw, absolute=False):
        """A per-head / per-row reduction: symbolic for the recognised spellings, else today's call on the materialised scores."""
        scope = _reduction_scope(name, args, kw)
        if scope is None:
            full = self._materialize()
            return getattr(full.abs() if absolute else full, name)(*args, **kw)
        return LazyStat(self, kind, 1.0, scope, (name, args, dict(kw), absolute))

    def amax(self, *args, **kw):
        return self._scoped(ops.STAT_MAX, "amax", args, kw)

    def amin(self, *args, **kw):
        return self._scoped(ops.STAT_MIN, "amin", args, kw)

    def sum(self, *args, **kw):
        if args or kw:
            return self._materialize().sum(*args, **kw)
        return self._shape_out(self._st()[:, 2])

    def mean(self, *args, **kw):
        if args or kw:
            return self._scoped(ops.STAT_MEAN, "mean", args, kw)
        return LazyStat(self, ops.STAT_MEAN)

    def var(self, *args, **kw):
        if args or kw:
            return self._materialize().var(*args, **kw)
        st, n = self._st(), self._count()
        var = (st[:, 3] - st[:, 2] * st[:, 2] / n) / max(n - 1, 1)   # unbiased, like torch.var
        return self._shape_out(var.clamp_min(0))

    def std(self, *args, **kw):
        if args or kw:
            return self._scoped(ops.STAT_STD, "std", args, kw)
        return LazyStat(self, ops.STAT_STD)

    def abs(self):
        return _AbsQK(self)

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return 3

    def numel(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    # -- escape hatch: the real tensor -----------------------------------------------------------
    def _materialize(self):
        if self._full is None:
            _warn_once("materialize", "weight_function uses qk beyond global reductions; materialising Q K^T "
                                      "(correct but slower than the fused reduction path)")
            B, N, C = self._q.shape
            h = self._heads
            qh = self._q.reshape(B, N, h, C // h).permute(0, 2, 1, 3)
            kh = self._k.reshape(B, -1, h, C // h).permute(0, 2, 3, 1)
            self._full = torch.matmul(qh, kh).reshape(B * h, N, -1)
        return self._full

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._materialize(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        conv = lambda a: a._materialize() if isinstance(a, QKProxy) else a  # noqa: E731
        return func(*[conv(a) for a in args], **{k: conv(v) for k, v in (kwargs or {}).items()})

    def __add__(self, other):
        return self._materialize() + other

    def __radd__(self, other):
        return other + self._materialize()

    def __sub__(self, other):
        return self._materialize() - other

    def __rsub__(self, other):
        return other - self._materialize()

    def __mul__(self, other):
        return self._materialize() * other

    def __rmul__(self, other):
        return other * self._materialize()

    def __truediv__(self, other):
        return self._materialize() / other

    def __rtruediv__(self, other):
        return other / self._materialize()

    def __pow__(self, other):
        return self._materialize() ** other

    def __neg__(self):
        return -self._materialize()

    def __getitem__(self, idx):
        return self._materialize()[idx]


class _LazyQuery:
    """`attn.to_q(hidden_states)` (:76), evaluated on first use. Shape / dtype / device are known without running it."""

    def __init__(self, attn, hidden_states, dtype):
        self.attn, self.hidden, self.value = attn, hidden_states, None
        self.shape = torch.Size((hidden_states.shape[0], hidden_states.shape[1], attn.to_q.weight.shape[0]))
        self.dtype, self.device = dtype, hidden_states.device

    @property
    def done(self):
        return self.value is not None

    def get(self):
        if self.value is None:
            self.value = self.attn.to_q(self.hidden)
            lo = self.attn.__dict__.get(LORA_ATTR)
            if lo is not None:
                _lora_update(lo, self.value, self.hidden, _Q)
        return self.value


class _AbsQK:
    """``qk.abs()``: its max / mean-free reductions follow from the signed statistics."""

    def __init__(self, proxy):
        self._p = proxy

    def max(self):
        return LazyStat(self._p, ops.STAT_ABSMAX)

    def amax(self, *args, **kw):
        return self._p._scoped(ops.STAT_ABSMAX, "amax", args, kw, absolute=True)

    def __getattr__(self, name):
        return getattr(self._p._materialize().abs(), name)


class ScaledW:
    """Lazy ``coeff * w`` handed to ``weight_function`` in place of the weight map ``w`` (:94, :106).

    Every shipped weight function is ``c0 * w * g(sigma) * reduce(qk)`` -- scalar (or per-image) factors times
    the constant map. Multiplying / dividing a ScaledW by Python numbers, 0-dim tensors or per-image
    ``[B,1,1,1]`` tensors only updates the coefficient; the fused kernel then receives the ORIGINAL map plus
    the coefficient vector (``bias_coeff``), so the [N, 77] product is never materialised (3-4 tiny elementwise
    launches per cross-attention layer and step saved). Any other use -- addition, indexing, torch functions,
    attribute access -- materialises the real tensor and the computation continues on it, unchanged.
    """
    __slots__ = ("w", "coeff", "stat")

    def __init__(self, w, coeff=1.0, stat=None):
        self.w, self.coeff, self.stat = w, coeff, stat      # value = w * coeff * (stat if stat is not None else 1)

    @staticmethod
    def _is_factor(x):
        if isinstance(x, (int, float)):
            return True
        return torch.is_tensor(x) and (x.dim() == 0 or (x.dim() == 4 and x.shape[1:] == (1, 1, 1)))

    def _scaled(self, factor, divide=False):
        if isinstance(factor, LazyStat):
            if not divide and self.stat is None and not torch.is_tensor(self.coeff):
                return ScaledW(self.w, self.coeff, factor)       # stays symbolic: the kernel forms the product
            factor = factor.materialize()
        if not self._is_factor(factor):
            return None
        if torch.is_tensor(factor):
            if self.stat is not None and self.stat.scope != SCOPE_IMAGE:
                return None                                      # a tensor factor beside a per-head / per-row statistic: the real tensors
            factor = factor.to(torch.float32)
            if self.stat is not None:                            # a second tensor factor: fall back to tensors
                return ScaledW(self.w, self.coeff * self.stat.materialize(), None)._scaled(factor, divide)
        c = self.coeff / factor if divide else self.coeff * factor
        return ScaledW(self.w, c, self.stat)

    def __mul__(self, other):
        r = self._scaled(other)
        return r if r is not None else self.materialize() * other

    __rmul__ = __mul__

    def __truediv__(self, other):
        r = self._scaled(other, divide=True)
        return r if r is not None else self.materialize() / other

    def __neg__(self):
        return ScaledW(self.w, -self.coeff, self.stat)

    def materialize(self):
        if self.stat is not None and self.stat.scope != SCOPE_IMAGE:
            return (self.w * self.coeff) * self.stat.materialize()      # (the order of `c * w * g(sigma) * qk.amax(...)` on tensors)
        c = self.coeff if self.stat is None else self.coeff * self.stat.materialize()
        return self.w * c

    # everything else behaves like the tensor it stands for
    def __add__(self, other): return self.materialize() + other
    def __radd__(self, other): return other + self.materialize()
    def __sub__(self, other): return self.materialize() - other
    def __rsub__(self, other): return other - self.materialize()
    def __rtruediv__(self, other): return other / self.materialize()
    def __pow__(self, other): return self.materialize() ** other
    def __getitem__(self, idx): return self.materialize()[idx]

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        conv = lambda a: a.materialize() if isinstance(a, ScaledW) else a  # noqa: E731
        return func(*[conv(a) for a in args], **{k: conv(v) for k, v in (kwargs or {}).items()})


class _ProbeProxy(QKProxy):
    """QKProxy without tensors behind it: the per-step re-evaluation of a weight function on the host (CoeffSlots.update) only
    needs the symbolic result; anything that would touch the scores says so."""

    def __init__(self, shape, dtype, device):   # noqa: super().__init__ deliberately not called (no q / k here)
        self._q_src = self._k = None
        self._heads, self._stats, self._full = 1, None, None
        self.shape, self.dtype, self.device = torch.Size(shape), dtype, device

    def _st(self):
        raise _NotSymbolic()

    def _materialize(self):
        raise _NotSymbolic()


class _NotSymbolic(Exception):
    pass


def _symbolic_scalar(result):
    """(STAT_* kind, python scalar) if a weight function's result is `c * w * stat(qk)` / `c * w` with a Python number c, else None."""
    if isinstance(result, ScaledW) and not torch.is_tensor(result.coeff) and torch.is_tensor(result.w):
        if result.stat is None:
            return ops.STAT_NONE, float(result.coeff)
        if result.stat.scope != SCOPE_IMAGE:
            return None         # (a per-head / per-row statistic: _symbolic_scoped)
        return result.stat.kind, float(result.coeff) * float(result.stat.scale)
    return None


def _symbolic_scoped(result):
    """(STAT_* kind, SCOPE_HEAD / SCOPE_ROW, python scalar) if a weight function's result is `c * w * stat(qk)` with a Python number c and a
    per-head or per-row statistic, else None."""
    if (isinstance(result, ScaledW) and not torch.is_tensor(result.coeff) and torch.is_tensor(result.w) and result.stat is not None
            and result.stat.scope != SCOPE_IMAGE):
        return result.stat.kind, result.stat.scope, float(result.coeff) * float(result.stat.scale)
    return None


class CoeffSlots:
    """hipGraph mode: one device word per cross-attention call site holds the Python scalar `c0 * g(sigma)` of the weight
    function (the kernels read it when they RUN: pww_cross_opts_t.coeff_scalar_dev), so ONE captured graph serves every
    denoise step and every weight function of the same shape -- the host re-evaluates the user's function per site and step
    on symbolic stand-ins (microseconds) and rewrites the words before each replay (reference: paint_with_words.py:479-482
    refreshes SIGMA / WEIGHT_FUNCTION in the dict every step). A weight function that is not of the form
    c * w * reduce(qk) marks the slots `unsupported`; the sampler then falls back to one graph per step.

    EVERY dict-context cross-attention call registers a site, also the ones whose weight function came back with no bias at all
    (a Python number, a 0-dim tensor, a bare statistic: kind NO_BIAS -- the captured graph then holds a bias-free kernel for that
    site). update() re-classifies every site each step and reports a change of class (no bias <-> symbolic, another statistic) as
    "re-capture" (a per-head / per-row statistic is its own class: kind = the pair (STAT_*, scope)): a graph captured while `lambda w, s, qk: 0` (or a sigma-thresholded function's zero branch) was in force is
    never replayed for a function that wants the bias."""
    MAX = 64
    NO_BIAS = -1

    def __init__(self, device):
        self.dev = torch.zeros(self.MAX, dtype=torch.float32, device=device)
        self.sites = []            # per call site, in call order: dict(kind, w, qk_shape, dtype)
        self.cursor = 0
        self.discover = True       # eager pass: sites are (re)registered and their words written in place
        self.unsupported = False

    def begin_forward(self):
        self.cursor = 0

    def reset(self):
        self.sites, self.cursor, self.discover, self.unsupported = [], 0, True, False

    def site(self, kind, scalar, w, qk_shape, dtype):
        """Called by pww_attention for a symbolic bias: returns the site's device word. In a discovery (eager) pass the word is
        written here; under capture it already holds this step's value (update() ran before)."""
        i = self.cursor
        self.cursor += 1
        if i >= self.MAX:
            self.unsupported = True
            return None
        if self.discover:
            rec = dict(kind=kind, w=w, qk_shape=tuple(qk_shape), dtype=dtype, device=self.dev.device)
            if i < len(self.sites):
                self.sites[i] = rec
            else:
                self.sites.append(rec)
            if kind != self.NO_BIAS:
                self.dev[i:i + 1].fill_(scalar)
        elif i >= len(self.sites) or self.sites[i]["kind"] != kind or self.sites[i]["w"] is not w:
            raise PwwHipError("cross-attention call sites changed between hipGraph capture passes (site %d)" % i)
        return self.dev[i:i + 1]

    @classmethod
    def classify(cls, result):
        """(kind, scalar) of a weight function's result: (STAT_*, c) for c * w [* stat(qk)], ((STAT_*, scope), c) for a per-head / per-row
        statistic, (NO_BIAS, 0.0) when the result adds
        nothing softmax can see (Python number, 0-dim tensor, bare statistic), None for anything else (a tensor-valued bias)."""
        sym = _symbolic_scalar(result)
        if sym is not None:
            return sym
        scoped = _symbolic_scoped(result)
        if scoped is not None:
            return (scoped[0], scoped[1]), scoped[2]        # the site's class is (statistic, scope)
        if isinstance(result, LazyStat) or isinstance(result, (int, float)) or (torch.is_tensor(result) and result.dim() == 0):
            return cls.NO_BIAS, 0.0
        return None

    def update(self, weight_function, sigma):
        """Re-evaluate the weight function for every registered site at this step's sigma and move the scalars to the device
        words (one pinned copy). Returns False if the function no longer has the captured structure (the caller re-captures)."""
        if not self.sites:
            return True
        vals = []
        for i, rec in enumerate(self.sites):
            w = rec["w"]
            try:
                res = weight_function(ScaledW(w) if torch.is_tensor(w) and _LAZY_W else w, sigma, _ProbeProxy(rec["qk_shape"], rec["dtype"], rec["device"]))
            except _NotSymbolic:
                return False
            sym = self.classify(res)
            if sym is None or sym[0] != rec["kind"]:
                return False
            vals.append(sym[1])
        # The host runs steps ahead of the GPU: the values ride in the arguments of one asynchronous launch (pww_store_f32). A
        # re-used pinned staging buffer would be overwritten with a later step's scalars before its copy executes, and a copy from
        # pageable memory is synchronous -- it would stop the host from running ahead at all (measured: -4 % images/s).
        ops.store_f32(self.dev, vals)
        return True


def _orig_weight_to_tokens(w_orig, n_tokens):
    """The reference's fallback when no CROSS_ATTENTION_WEIGHT_<N> key exists (:96-101): bilinear
    (align_corners=True) by 1/sqrt(H*W/N), then 1-D nearest to N -- pww_resize_tokens on the device map. A batched
    [n, H, W, T] map (paint_with_words_batch) gives [n, 1, N, T]."""
    if w_orig.dim() == 4:
        return torch.stack([ops.resize_tokens(w, n_tokens) for w in w_orig], dim=0).unsqueeze(1)
    return ops.resize_tokens(w_orig, n_tokens)


def refresh_orig_cache(context):
    """Recompute the cached fallback maps of a request context IN PLACE (hipGraph mode: a new color map was copied into
    the static CROSS_ATTENTION_WEIGHT_ORIG tensor; the captured graphs read the resized maps by address)."""
    cache = context.get("_PWW_ORIG_CACHE")
    if not cache:           # no layer took the fallback: the full-resolution map is not even built (conditioning.PwWContext)
        return
    w = context.get("CROSS_ATTENTION_WEIGHT_ORIG")
    if not torch.is_tensor(w):
        return
    for n_img, t in cache.items():
        t.copy_(_orig_weight_to_tokens(w, n_img))


def _half(t, like_dtype):
    """q/k/v must be fp16/bf16 for the MFMA path. The reference runs under autocast (fp16 matmuls,
    :60); an fp32 module without autocast is cast to bf16 with a one-time warning."""
    if t.dtype in _HALF:
        return t
    _warn_once("cast", "pww_hip attention received %s activations; casting to %s for the MFMA kernels "
                       "(the reference computes this path in fp16 under autocast)" % (t.dtype, like_dtype))
    return t.to(like_dtype)


def _compute_dtype(attn):
    """dtype the projections run in: the autocast dtype under `torch.autocast("cuda")` (the reference's inj_forward and
    paint_with_words are decorated with it, :60 / :392: fp16 matmuls whatever the module dtype), else the weights' dtype."""
    if torch.is_autocast_enabled():
        return torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
    return attn.to_q.weight.dtype


def _fused_weight(attn, names, dtype=None):
    """Concatenated projection weight ([sum C_out, C_in]) of bias-free Linear layers in `dtype` (default: as stored), cached on
    the module and rebuilt when any source weight changes (one GEMM instead of three / two)."""
    mods = [getattr(attn, n) for n in names]
    if any(getattr(m, "bias", None) is not None for m in mods):
        return None
    ws = [m.weight for m in mods]
    dtype = dtype or ws[0].dtype
    key = tuple([(w.data_ptr(), w._version, w.dtype, w.device) for w in ws]) + (dtype,)
    cache = attn.__dict__.setdefault("_pww_fused", {})
    ent = cache.get(names)
    if ent is None or ent[0] != key:
        ent = (key, torch.cat([w.detach().to(dtype) for w in ws], dim=0).contiguous())
        cache[names] = ent
    return ent[1]


def refresh_kv_cache(context):
    """Recompute every cached fused K|V projection of a request context IN PLACE (hipGraph mode: the captured
    graphs read these tensors by address, and the context tensor was just overwritten with a new request)."""
    cache = context.get(KV_CACHE)
    if not cache:
        return
    ctx = context["CONTEXT_TENSOR"]
    for attn, kv in cache.values():
        w = _fused_weight(attn, ("to_k", "to_v"), kv.dtype)
        lo = attn.__dict__.get(LORA_ATTR)
        if lo is None:
            kv.copy_(F.linear(ctx.to(w.dtype), w))
        else:       # the adapted K|V of this request's rows: the assignment was written before (sampler)
            x = ctx.to(w.dtype)
            x = x.expand(kv.shape[0], -1, -1) if x.shape[0] != kv.shape[0] else x
            kv.copy_(_lora_update(lo, F.linear(x, w), x, _KV))


def pww_attention(attn, hidden_states, context=None):
    """Core of inj_forward (:63-118): projections -> [optional bias] -> fused attention, returning the
    merged-head [B, N, heads*D] tensor BEFORE the output projection."""
    return _attention(attn, hidden_states, context, None)[0]


def _attention_and_out(attn, hidden_states, context):
    """inj_forward's :63-123: the attention and to_out[0] (to_out[1], the dropout, is the caller's)."""
    lin = attn.to_out[0]
    lo = attn.__dict__.get(LORA_ATTR)
    out, projected = _attention(attn, hidden_states, context, lin if FUSE_TO_OUT and lo is None else None)
    if projected:
        return out
    if lo is None:
        return lin(out.to(lin.weight.dtype))
    x = out.to(lin.weight.dtype)
    return _lora_update(lo, lin(x), x, _OUT)


def _attention(attn, hidden_states, context, out_linear):
    """-> (tensor, projected): with `out_linear` (the layer's to_out[0]) and a layer pww_cross_attn_fwd_parts_out covers, the
    projection is applied inside the attention launch and `projected` is True."""
    p = _project(attn, hidden_states, context)
    return _launch(attn, p, _plan(attn, p, out_linear), out_linear)


# What _project hands on. query: in the compute dtype `cdt` like key / value, or still deferred (a _LazyQuery: see _query); ctx: a PwW dict or None
_Proj = collections.namedtuple("_Proj", "hidden query key value cdt pdt lo ctx")
# What one attention call launches, decided once by _plan. family: "none" (nothing softmax can see: a number, a 0-dim tensor, a bare
# statistic), "scoped" (c * w * a per-head / per-row statistic on libpww_hip_scope.so; scoped = (kind, scope, scalar)), "symbolic" (c * w
# [* stat(qk)]: the map, stat = (statistics [B, 4] | None, STAT_* kind, Python scalar) and what the statistic's launch needs), "vector" (the
# map with a per-row coefficient vector) or "materialised" (a tensor). bias_coeff: fp32 [B], the row gate or the vector family's coefficient.
_Plan = collections.namedtuple("_Plan", "family query bias bias_coeff stat parts scratch coeff_dev bias_cols compact gated scoped",
                               defaults=(None, None, None, None, None, None, 0, None, 0, None))


def _query(p):
    """The query of a projection in the compute dtype; a deferred to_q runs here. Every plan asks once."""
    q = p.query
    return _half(q.get(), p.cdt) if isinstance(q, _LazyQuery) else q


def _qk_shape(attn, p):
    return (p.hidden.shape[0] * attn.heads, p.hidden.shape[1], p.key.shape[1])


def _project(attn, hidden_states, context):
    """Step 1 of _attention: context parsing, dtype alignment and one of three projection strategies, each followed by the layer's LoRA update --
    q|k|v in one GEMM (self-attention), k|v in one GEMM with the query deferred (cross-attention), or the module's own three."""
    ctx = None
    if context is None:
        context_tensor = hidden_states
    elif isinstance(context, dict) or hasattr(context, "keys"):
        context_tensor, ctx = context["CONTEXT_TENSOR"], context
    else:                   # plain tensor context: vanilla pipelines keep working (the reference's try/except, :65-69)
        context_tensor = context
    if not hidden_states.is_cuda:
        raise PwwHipError("pww_hip attention needs HIP tensors (got %s); the CPU restatement lives in oracle/ "
                          "and is test-only" % hidden_states.device)
    wq = attn.to_q.weight
    wdt, C = wq.dtype, wq.shape[0]
    if context_tensor.dtype != wdt and not torch.is_autocast_enabled():
        context_tensor = context_tensor.to(wdt)   # text encoder is fp32 in the reference (:171)
    if hidden_states.dtype != wdt and not torch.is_autocast_enabled():
        hidden_states = hidden_states.to(wdt)
    # Fused projections in the dtype the reference's path computes in: under torch.autocast("cuda") (how the reference runs, :60 / :392) that
    # is the autocast dtype, and the concatenated weights are kept in it, so autocast has nothing left to cast per call.
    pdt = _compute_dtype(attn)
    lo = attn.__dict__.get(LORA_ATTR)
    if lo is not None and context is not None and context_tensor.shape[0] != hidden_states.shape[0]:
        context_tensor = context_tensor.expand(hidden_states.shape[0], -1, -1)      # one row of K|V per row of the assignment
    if context is None and (w_qkv := _fused_weight(attn, _QKV, pdt)) is not None:
        qkv = F.linear(hidden_states.to(pdt), w_qkv)            # self-attention: ONE GEMM, q/k/v are strided views
        if lo is not None:
            _lora_update(lo, qkv, hidden_states.to(pdt), _QKV)
        query, key, value = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    elif context is not None and (w_kv := _fused_weight(attn, _KV, pdt)) is not None:
        if ctx is not None:
            query = _LazyQuery(attn, hidden_states, pdt if pdt in _HALF else torch.bfloat16)      # deferred: see _plan_symbolic
        else:
            query = attn.to_q(hidden_states)
            if lo is not None:
                _lora_update(lo, query, hidden_states, _Q)
        kv_cache = ctx.get(KV_CACHE) if ctx is not None else None
        ent = kv_cache.get(id(attn)) if kv_cache is not None else None
        if ent is None:
            kv = F.linear(context_tensor.to(pdt), w_kv)         # cross-attention: K|V in one GEMM ...
            if lo is not None:
                _lora_update(lo, kv, context_tensor.to(pdt), _KV)
            if kv_cache is not None:
                kv_cache[id(attn)] = (attn, kv)                 # ... and once per request: the prompt is constant over the steps
        else:
            kv = ent[1]
        key, value = kv[..., :C], kv[..., C:]
    else:
        query = attn.to_q(hidden_states)
        key = attn.to_k(context_tensor)
        value = attn.to_v(context_tensor)
        if lo is not None:
            _lora_update(lo, query, hidden_states, _Q)
            _lora_update(lo, key, context_tensor, ("to_k",))
            _lora_update(lo, value, context_tensor, ("to_v",))
    lazy = isinstance(query, _LazyQuery)
    src = key if lazy else query
    cdt = src.dtype if src.dtype in _HALF else torch.bfloat16
    return _Proj(hidden_states, query if lazy else _half(query, cdt), _half(key, cdt), _half(value, cdt), cdt, pdt, lo, ctx)


def _plan(attn, p, out_linear):
    """Step 2 of _attention: look the weight map up, call the user's weight function and classify what it returned. The launches that produce
    a statistic's partials and the hipGraph slot bookkeeping happen here, in call order."""
    ctx = p.ctx
    if ctx is None:
        return _Plan("none", p.query)
    gate = ctx.get(ROW_GATE)   # folded CFG batches: per-row coefficient (1 = cond row; uncond row: 0, or negative_strength with negative regions)
    f = ctx["WEIGHT_FUNCTION"]
    n_img = p.hidden.shape[1]
    try:
        w = ctx[f"CROSS_ATTENTION_WEIGHT_{n_img}"]
    except KeyError:        # the reference's fallback (:96-101) on the full-resolution map, kept per token count
        w = ctx["CROSS_ATTENTION_WEIGHT_ORIG"]
        if not isinstance(w, int):
            cache = ctx.setdefault("_PWW_ORIG_CACHE", {})
            if n_img not in cache:
                cache[n_img] = _orig_weight_to_tokens(w, n_img)
            w = cache[n_img]
    lazy_w = ScaledW(w) if torch.is_tensor(w) and _LAZY_W else w
    bias = f(lazy_w, ctx["SIGMA"], QKProxy(p.query, p.key, attn.heads))
    slots = ctx.get(COEFF_SLOTS)
    if isinstance(bias, LazyStat):     # a bare statistic: a per-image constant on every logit of a row cancels in softmax
        bias = None
    scoped = _symbolic_scoped(bias)
    if scoped is not None:
        # c0 * w * g(sigma) * reduce(qk over one head / one row): libpww_hip_scope.so forms the coefficient; what it declines goes on as tensors
        kind, scope, scalar = scoped
        if _scoped_route(attn, p.key, bias.w, kind, scope, ctx.get(ATTN_RECORDER), out_linear):
            query, coeff_dev, parts = _query(p), None, None
            if slots is not None and not slots.unsupported:
                coeff_dev = slots.site((kind, scope), scalar, bias.w, _qk_shape(attn, p), p.cdt)
            if scope == SCOPE_HEAD:
                parts = ops.scope_head_parts(query, p.key, attn.heads, kind, gate=gate)
            return _Plan("scoped", query, bias.w, gate, None, parts, None, coeff_dev, 0, None, 0, scoped)
        bias = bias.materialize()
    sym = _symbolic_scalar(bias)
    if sym is not None and (bias.stat is not None or slots is not None):
        return _plan_symbolic(attn, p, bias, sym, gate, slots, w)
    family, coeff = "materialised", gate
    if isinstance(bias, ScaledW):      # coeff * w with a tensor coefficient: keep the map, pass the coefficient vector to the kernel
        if slots is not None:
            slots.unsupported = True   # (sigma reached the kernel arguments through torch ops: one graph per step)
        family, coeff, bias = "vector", _row_coefficients(bias, gate, p.hidden), bias.w
    return _checked(attn, p, slots, w, _Plan(family, _query(p), bias, coeff))


def _plan_symbolic(attn, p, bias, sym, gate, slots, w):
    """c0 * w * g(sigma) [* reduce(qk)]: map, statistic selector and scalar (hipGraph mode: a device word) go to the kernel as they are."""
    kind, scalar = sym
    ctx, hidden, key, pdt, w_map = p.ctx, p.hidden, p.key, p.pdt, bias.w
    n_img, M = hidden.shape[1], key.shape[1]
    bias_cols = int(ctx.get(BIAS_COLS, 0) or 0)
    gated = int(ctx.get(GATED_ROWS, 0) or 0) if gate is not None else 0
    coeff_dev = parts = scratch = query = None
    wc, ci = ctx.get(COMPACT_W + str(n_img)), ctx.get(COMPACT_IDX)
    compact = (wc, ci) if torch.is_tensor(wc) and torch.is_tensor(ci) and ctx.get(f"CROSS_ATTENTION_WEIGHT_{n_img}") is w_map else None
    if slots is not None and not slots.unsupported:
        coeff_dev = slots.site(kind, scalar, w_map, _qk_shape(attn, p), p.cdt)
    have_stats = bias.stat is not None and bias.stat._proxy._stats is not None
    stat = (None, kind, scalar)
    short = M <= ops.FUSED_MAX_KEYS
    if have_stats or not (short or ops.long_keys(M)):
        # the weight function already forced the statistics to exist as a tensor, or more keys than a pass-2-only launch takes
        stat = (bias.stat.stats() if bias.stat is not None else None, kind, scalar)
    else:
        # Q and the statistic's partials from ONE launch (to_q GEMM, statistic in its epilogue): the query is untouched, the GEMM covers the shape
        if (short and p.lo is None and qproj_route(hidden.shape[-1], hidden.shape[-1] // attn.heads) and isinstance(p.query, _LazyQuery)
                and not p.query.done and kind != ops.STAT_NONE and pdt in _HALF and key.dtype == pdt and getattr(attn.to_q, "bias", None) is None):
            wq = _fused_weight(attn, _Q, pdt)
            x = hidden if hidden.dtype == pdt else hidden.to(pdt)
            if wq is not None and ops.qproj_parts(x, wq, key, attn.heads) > 0:
                query, parts = ops.qproj_stat(x, wq, key, attn.heads, kind, gate=gate)
        if parts is None and short and FUSED_CROSS:
            scratch = attn.__dict__.get("_pww_fused_scratch")
            if scratch is None:
                scratch = attn.__dict__["_pww_fused_scratch"] = ops.FusedScratch()
        elif parts is None and kind != ops.STAT_NONE:
            # the default for every layer the GEMM-epilogue route does not take: stock to_q, one small launch for the statistic's partials over
            # the finished Q (libpww_hip_long.so's for a prompt encoded in 2 or 3 chunks), pass-2-only attention; `c * w` needs no partials
            query = _query(p)
            parts = (ops.qk_parts if short else ops.long_qk_parts)(query, key, attn.heads, kind, gate=gate, gated=gated)
    if query is None:
        query = _query(p)
    return _checked(attn, p, slots, w, _Plan("symbolic", query, w_map, gate, stat, parts, scratch, coeff_dev, bias_cols, compact, gated))


def _row_coefficients(bias, gate, hidden):
    """The fp32 [B] coefficient vector of a ScaledW with a tensor (or, outside hipGraph mode, Python) coefficient, times the row gate."""
    if bias.stat is not None:
        bias = ScaledW(bias.w, bias.coeff * bias.stat.materialize())
    c, B = bias.coeff, hidden.shape[0]
    if torch.is_tensor(c):
        coeff = c.reshape(-1).to(torch.float32)
        coeff = coeff.expand(B) if coeff.numel() == 1 else coeff
    else:
        coeff = torch.full((B,), float(c), dtype=torch.float32, device=hidden.device)
    return coeff if gate is None else coeff * gate


def _checked(attn, p, slots, w, plan):
    """`plan` if its bias is a tensor softmax can see, else the "none" plan. hipGraph slots: a call without a bias registers a NO_BIAS site (the
    graph holds a bias-free kernel there), a bias without `stat` depends on sigma through torch ops and marks the slots unsupported."""
    bias = plan.bias
    if isinstance(bias, QKProxy):
        plan = plan._replace(bias=(bias := bias._materialize()))
    if not torch.is_tensor(bias) or bias.dim() == 0:       # a constant on every logit of a row cancels in softmax (the unconditional pass returns 0.0, :493)
        if slots is not None and not slots.unsupported:
            slots.site(CoeffSlots.NO_BIAS, 0.0, w, _qk_shape(attn, p), p.cdt)
        return _Plan("none", plan.query)
    if slots is not None and plan.stat is None:
        slots.unsupported = True
    return plan


def _launch(attn, p, plan, out_linear):
    """Step 3 of _attention: the scoped launch, the attention + to_out launch or ops.attention -- with a recorder in the context, followed by
    one probabilities launch with the same q / k / map / coefficient inputs (pww_hip.record_attention_maps)."""
    family, query, bias, gate, stat, parts, scratch, coeff_dev, bias_cols, compact, gated, scoped = plan
    key, value = p.key, p.value
    if family == "scoped":
        return ops.attention_scoped(query, key, value, attn.heads, attn.scale, bias, *scoped, gate=gate, parts=parts, coeff_dev=coeff_dev), False
    rec = p.ctx.get(ATTN_RECORDER) if p.ctx is not None else None
    if family == "none":
        out = ops.attention(query, key, value, attn.heads, attn.scale)
        if rec is not None:
            _record_probs(rec, attn, p.ctx, query, key, None, None, None, None)
        return out, False
    if (out_linear is not None and stat is not None and stat[0] is None and scratch is None and key.shape[1] <= ops.FUSED_MAX_KEYS
            and out_linear.weight.dtype == query.dtype and ops.attention_out_supported(query, key, attn.heads, bias, out_linear.weight, bias_cols)):
        # row f-1 (opt-in, FUSE_TO_OUT): attention + to_out[0] in one launch; the dense map serves (the compact form is the general kernel's)
        wb = out_linear.bias
        if rec is not None:
            _warn_once("record_to_out", "attention maps: the attention + to_out launch of the experiments library is not recorded")
        return ops.attention_out(query, key, value, attn.heads, attn.scale, bias, out_linear.weight, wb if wb is None else wb.to(query.dtype),
                                 bias_coeff=gate, stat=stat, parts=parts, coeff_dev=coeff_dev, bias_cols=bias_cols, gated=gated), True
    if rec is None:
        return ops.attention(query, key, value, attn.heads, attn.scale, bias=bias, bias_coeff=gate, stat=stat, scratch=scratch,
                             coeff_dev=coeff_dev, bias_cols=bias_cols, compact=compact, gated=gated, parts=parts), False
    # recording: the "parts" and "long" routes fold their statistic inside the attention launch, which is asked to hand the folded fields out
    route = ops.attention_route(True, stat, scratch, parts, key.shape[1])
    folds = route in ("parts", "long")
    stats_out = None
    if folds and stat[1] != ops.STAT_NONE and not rec.muted:
        stats_out = torch.empty((query.shape[0], 4), dtype=torch.float64, device=query.device)
    out = ops.attention(query, key, value, attn.heads, attn.scale, bias=bias, bias_coeff=gate, stat=stat, scratch=scratch, stats_out=stats_out,
                        coeff_dev=coeff_dev, bias_cols=bias_cols, compact=compact, gated=gated, parts=parts)
    if route == "fused":
        _warn_once("record_fused", "attention maps: the in-launch statistic route of the experiments library (PWW_FUSED_CROSS=1) is not recorded")
    else:       # "plain": c[b] = gate[b]; "stat": the [B, 4] statistics came with the call; "parts" / "long": the launch handed them out
        _record_probs(rec, attn, p.ctx, query, key, bias, gate, (stats_out, stat[1], stat[2]) if folds else stat, coeff_dev)
    return out, False


def _scoped_route(attn, key, w_map, kind, scope, rec, out_linear):
    """Does libpww_hip_scope.so take this call? (c * w * a per-head / per-row statistic: at most FUSED_MAX_KEYS keys, half-precision
    q / k / v, no attention-map recorder, not the attention + to_out launch, the switch on, the library there, a shape it supports.)"""
    if not SCOPED_STATS or rec is not None or out_linear is not None or key.dtype not in _HALF:
        return False
    M, D = key.shape[1], key.shape[2] // attn.heads
    if M > ops.FUSED_MAX_KEYS or D % 8 or D > ops.MAX_HEAD_DIM or w_map.stride(-1) != 1 or (kind == ops.STAT_STD and M < 2):
        return False
    return ops.scoped_available()


def _record_probs(rec, attn, context, query, key, bias, coeff, stat, coeff_dev):
    """One ops.attention_probs launch behind the attention launch of a recorded cross-attention call: the head-averaged probabilities of the
    conditional rows, added into the recorder's accumulator for this token count (or layer)."""
    B, N, M = query.shape[0], query.shape[1], key.shape[1]
    if M > ops.LONG_MAX_KEYS:
        _warn_once("record_keys", "attention maps: cross-attention over %d > %d keys is not recorded" % (M, ops.LONG_MAX_KEYS))
        return
    cond_rows = int(context.get(COND_ROWS, 0) or context.get(GATED_ROWS, 0) or 0) if context.get(ROW_GATE) is not None else 0
    tgt = rec.target(attn, B, N, M, cond_rows, query.device)
    if tgt is None:
        return
    buf, images = tgt
    if stat is not None and stat[0] is None and stat[1] != ops.STAT_NONE:
        raise PwwHipError("attention maps: the attention launch's statistics are missing for this call")
    ops.attention_probs(query, key, attn.heads, attn.scale, bias=bias, bias_coeff=coeff, stat=stat, coeff_dev=coeff_dev,
                        images=images if images < B else 0, out=buf, accumulate=True)


def inj_forward(self, hidden_states, context=None, mask=None):
    """Drop-in for the reference's ``inj_forward`` (:60-125): same signature, same context protocol
    ({None | Tensor | dict with CONTEXT_TENSOR / CROSS_ATTENTION_WEIGHT_* / SIGMA / WEIGHT_FUNCTION}),
    ``mask`` accepted and ignored like the reference (:61)."""
    out = _attention_and_out(self, hidden_states, context)
    out = self.to_out[1](out)
    return out


def install(unet):
    """The reference's plug (:193-195): for every module whose class is named ``CrossAttention``
    replace ``__call__`` at class level. Returns the number of modules found."""
    n = 0
    for module in unet.modules():
        if module.__class__.__name__ == "CrossAttention":
            module.__class__.__call__ = inj_forward
            n += 1
    # the blocks around the attention path (row a17): GroupNorm (+ time-embedding addend, + SiLU) on the HIP kernels, per instance
    from . import blocks
    blocks.install_blocks(unet)
    return n


def uninstall(unet):
    from . import blocks
    blocks.uninstall_blocks(unet)
    for module in unet.modules():
        cls = module.__class__
        if cls.__name__ == "CrossAttention" and cls.__dict__.get("__call__") is inj_forward:
            del cls.__call__


class PwWAttnProcessor:
    """Attention-processor form of the same op for diffusers >= 0.12 ``Attention`` modules
    (``unet.set_attn_processor(PwWAttnProcessor())``): ``encoder_hidden_states`` carries the PwW dict."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, **kwargs):
        residual = hidden_states
        spatial = hidden_states.dim() == 4
        if spatial:
            b, c, h, w = hidden_states.shape
            hidden_states = hidden_states.view(b, c, h * w).transpose(1, 2)
        ctx = encoder_hidden_states
        if getattr(attn, "norm_cross", None) is not None and ctx is not None:
            if isinstance(ctx, dict):
                normed = attn.norm_encoder_hidden_states(ctx["CONTEXT_TENSOR"])
                ctx = ctx.copy()          # (PwWContext.copy keeps the entries that are built on first access: CROSS_ATTENTION_WEIGHT_ORIG; dict(ctx) would drop them)
                ctx["CONTEXT_TENSOR"] = normed
            else:
                ctx = attn.norm_encoder_hidden_states(ctx)
        out = _attention_and_out(attn, hidden_states, ctx)
        out = attn.to_out[1](out)
        if spatial:
            out = out.transpose(-1, -2).reshape(b, c, h, w)
        if getattr(attn, "residual_connection", False):
            out = out + residual
        return out / getattr(attn, "rescale_output_factor", 1.0)
