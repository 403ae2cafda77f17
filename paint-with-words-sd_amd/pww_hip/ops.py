"""Torch-facing wrappers of the C ABI: tensors in, tensors out, launched on torch's current stream.

PyTorch here is plumbing (device memory from the caching allocator, the current HIP stream, dtype /
stride bookkeeping); all arithmetic happens in libpww_hip.so. Every function requires tensors on a
HIP device and raises if the library is missing -- there is no fallback path.
"""
import ctypes

import torch

from . import _lib
from ._lib import AttnDesc, CrossOpts, ProbsDesc, QprojDesc, Region, PwwHipError

_DT = {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise PwwHipError("pww_hip ops need tensors on a HIP device (got %s); there is no CPU path" % t.device)


def _rows_ok(t):
    """last dim contiguous, rows 16-byte aligned"""
    return t.stride(-1) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0


def _desc(q, k, v, o, heads, scale):
    if q.dim() != 3 or k.dim() != 3 or (v is not None and v.dim() != 3):
        raise PwwHipError("q/k/v must be [batch, tokens, heads*dim] tensors")
    B, N, C = q.shape
    M = k.shape[1]
    if C % heads:
        raise PwwHipError("channels %d not divisible by heads %d" % (C, heads))
    if k.shape[2] != C or k.shape[0] not in (1, B):
        raise PwwHipError("key shape %s does not match query shape %s" % (tuple(k.shape), tuple(q.shape)))
    if v is not None and tuple(v.shape) != tuple(k.shape):
        raise PwwHipError("value shape %s differs from key shape %s" % (tuple(v.shape), tuple(k.shape)))
    if M < 1 or N < 1 or B < 1:
        raise PwwHipError("empty attention problem (B=%d N=%d M=%d)" % (B, N, M))
    D = C // heads
    d = AttnDesc()
    d.dtype = _DT[q.dtype]
    d.B, d.H, d.N, d.M, d.D = B, heads, N, M, D
    d.q_stride[:] = [q.stride(0), D, q.stride(1)]
    kb = k.stride(0) if k.shape[0] == B and B > 1 else 0     # a batch-1 context is shared by every image
    d.k_stride[:] = [kb, D, k.stride(1)]
    if v is not None:
        d.v_stride[:] = [v.stride(0) if v.shape[0] == B and B > 1 else 0, D, v.stride(1)]
    if o is not None:
        d.o_stride[:] = [o.stride(0), D, o.stride(1)]
    d.scale = float(scale)
    return d


def _prep(t):
    if t.dtype not in _DT:
        raise PwwHipError("dtype %s unsupported (float16 / bfloat16)" % t.dtype)
    return t if _rows_ok(t) else t.contiguous()


STAT_NONE, STAT_MAX, STAT_MIN, STAT_MEAN, STAT_STD, STAT_ABSMAX, STAT_ALL = 0, 1, 2, 3, 4, 5, 6   # PWW_STAT_* of include/pww_hip.h
FUSED_MAX_KEYS = 128   # pww_cross_attn_fwd_fused: one K/V stage
MAX_HEAD_DIM = _lib.MAX_HEAD_DIM
LONG_MAX_KEYS = _lib.LONG_MAX_KEYS   # libpww_hip_long.so: the same pair of launches for FUSED_MAX_KEYS < M <= 256 (prompts encoded in 2 / 3 chunks)
COMPACT_MAX_R = 32     # pww_cross.hip: the compact form holds at most 32 non-zero columns


class FusedScratch:
    """EXPERIMENTS LIBRARY (libpww_hip_experiments.so; tests and A/B tools): device buffers of pww_cross_attn_fwd_fused for one call site (one attention layer): the persistent state words
    (zeroed ONCE here -- the kernel leaves them zero after every launch, so captured hipGraphs replay without a memset
    node) and the scratch of the two-launch path. Allocated outside stream capture (the first, eager call of a layer
    creates them) and kept alive by their owner, because captured graphs hold their addresses: a buffer that has to grow
    is RETIRED, never freed (graphs captured for the smaller geometry keep replaying into it)."""

    def __init__(self):
        self.state = None
        self.ws = None
        self._err_index = 0
        self._retired = []
        self._err_sites = {}       # id(state buffer) -> (buffer, {error-word indices of every geometry launched into it})

    def _alloc(self, current, nbytes, device, zero):
        if current is not None and current.device == device and current.numel() * 8 >= nbytes:
            return current
        if torch.cuda.is_current_stream_capturing():
            raise PwwHipError("fused cross-attention buffers must exist before hipGraph capture (run one eager call first)")
        if current is not None:
            self._retired.append(current)
        n = (nbytes + 7) // 8
        return (torch.zeros if zero else torch.empty)((n,), dtype=torch.int64, device=device)

    def ensure(self, lib, d, device):
        lib = _lib.load_experiments()      # (the hand-off form's size queries live where the launch lives)
        self.state = self._alloc(self.state, int(lib.pww_cross_fused_state_bytes(ctypes.byref(d))), device, True)
        self.ws = self._alloc(self.ws, int(lib.pww_cross_fused_workspace_bytes(ctypes.byref(d))), device, False)
        self._err_index = d.B * d.H + d.B
        self._err_sites.setdefault(id(self.state), (self.state, set()))[1].add(self._err_index)
        return self.state, self.ws

    def error_word(self):
        """The error word of the last call's geometry as a 0-dim device tensor (non-zero: a hand-off inside the fused kernel
        timed out and the affected outputs are NaN), or None before the first call. No synchronisation."""
        return None if self.state is None else self.state.view(torch.int32)[self._err_index]

    def error_words(self):
        """The error words of EVERY geometry this call site was ever launched with, retired buffers included (graphs captured for
        a smaller geometry keep replaying into them; a layer that alternates between batch geometries has its word at another
        index each time): a list of 0-dim device tensors. No synchronisation."""
        return [buf.view(torch.int32)[i] for buf, idxs in self._err_sites.values() for i in sorted(idxs)]

    def error(self):
        """True if a hand-off timed out (synchronises). The state words must then be re-zeroed: `reset()`."""
        words = self.error_words()
        return bool(words) and bool(torch.stack(words).ne(0).any().item())

    def reset(self):
        for t in [self.state] + self._retired:
            if t is not None:
                t.zero_()


class FusedErrorWatch:
    """check_fused_errors without stopping the host: after a request's last launch the error words of all layers are reduced on the
    device and copied to a pinned host flag behind an event (`post`); `poll` looks at the flags whose event has completed -- or
    waits for all of them -- and raises like check_fused_errors. The sampler posts at the end of every request and polls at the
    start of the next one, the PIL-returning entry points poll with wait=True after the decode they synchronise on anyway: the
    host keeps running ahead of the GPU between requests (a synchronous check after every image costs ~3 % images/s at batch 1:
    the next request's conditioning would start only when the GPU is idle)."""

    def __init__(self):
        self.pending = []

    def post(self, modules):
        scratches = [m.__dict__["_pww_fused_scratch"] for m in modules if "_pww_fused_scratch" in getattr(m, "__dict__", {})]
        words = [w for s in scratches for w in s.error_words()]
        if not words:
            return False
        flag = torch.stack(words).ne(0).any().to(torch.int32)
        host = torch.empty((), dtype=torch.int32).pin_memory()
        host.copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev, host, scratches))
        return True

    def poll(self, wait=False):
        while self.pending:
            ev, host, scratches = self.pending[0]
            if wait:
                ev.synchronize()
            elif not ev.query():
                return
            self.pending.pop(0)
            if int(host.item()) != 0:
                torch.cuda.synchronize()
                for s in scratches:
                    s.reset()
                self.pending.clear()
                raise PwwHipError(_TIMEOUT_MESSAGE)


_TIMEOUT_MESSAGE = ("a fused cross-attention launch timed out waiting for its own workgroups (the GPU is shared with another process or "
                    "stream?); its outputs are NaN and were discarded. State re-zeroed. Set PWW_FUSED_CROSS=0 to use the two-launch "
                    "path on a shared device.")


def check_fused_errors(modules):
    """One device -> host read for a whole request: raise PwwHipError if any fused cross-attention launch of the given
    modules' scratch buffers timed out in its hand-off (the launch needs every workgroup resident at once: another process or
    stream holding compute units can starve it; PWW_FUSED_CROSS=0 selects the two-launch path). Dirty state is re-zeroed so
    that the next request starts clean."""
    scratches = [m.__dict__["_pww_fused_scratch"] for m in modules if "_pww_fused_scratch" in getattr(m, "__dict__", {})]
    words = [w for s in scratches for w in s.error_words()]
    if not words:
        return
    if bool(torch.stack(words).ne(0).any().item()):
        torch.cuda.synchronize()
        for s in scratches:
            s.reset()
        raise PwwHipError(_TIMEOUT_MESSAGE)


def _cross_opts(B, N, coeff_dev, bias_cols, compact, gated=0):
    """pww_cross_opts_t for the *_ex entry points (None if nothing optional is asked for). The struct holds device addresses, not
    references: the compact views made here ride on it as `op.keep`, so they live as long as the caller holds the struct."""
    if coeff_dev is None and not bias_cols and compact is None and not gated:
        return None
    op = CrossOpts()
    op.size = ctypes.sizeof(CrossOpts)
    op.bias_cols = int(bias_cols or 0)
    op.gated_images = int(gated or 0)
    if coeff_dev is not None:
        if coeff_dev.dtype != torch.float32 or coeff_dev.numel() != 1 or not coeff_dev.is_cuda:
            raise PwwHipError("coeff_dev must be a one-element float32 device tensor")
        op.coeff_scalar_dev = coeff_dev.data_ptr()
    if compact is not None:
        wc, idx = compact
        if wc.dtype != torch.float32 or idx.dtype != torch.int32 or wc.stride(-1) != 1 or idx.stride(-1) != 1:
            raise PwwHipError("compact bias: float32 values and int32 column indices, innermost stride 1")
        if wc.dim() == 2:
            wc = wc.unsqueeze(0)
        if idx.dim() == 1:
            idx = idx.unsqueeze(0)
        R = wc.shape[-1]
        if wc.shape[1] != N or wc.shape[0] not in (1, B) or idx.shape[-1] != R or idx.shape[0] not in (1, B):
            raise PwwHipError("compact bias shapes %s / %s do not fit B=%d N=%d" % (tuple(wc.shape), tuple(idx.shape), B, N))
        op.bias_compact, op.col_idx, op.R = wc.data_ptr(), idx.data_ptr(), R
        op.compact_stride[:] = [wc.stride(0) if wc.shape[0] == B and B > 1 else 0, wc.stride(1)]
        op.col_idx_stride = idx.stride(0) if idx.shape[0] == B and B > 1 else 0
        op.keep = (wc, idx)
    return op


def _opt_ref(op):
    return ctypes.byref(op) if op is not None else None


def _bias_view(bias, d):
    """The fp32 [B, heads, N, M] view of a bias that broadcasts to it, its strides entered into the descriptor."""
    if bias.dtype != torch.float32:
        bias = bias.float()
    if bias.dim() == 3 and bias.shape[0] == d.B * d.H and d.B * d.H != 1:
        bias = bias.reshape(d.B, d.H, bias.shape[1], bias.shape[2])
    bias = torch.broadcast_to(bias, (d.B, d.H, d.N, d.M))  # view: broadcast axes get stride 0
    d.bias_stride[:] = list(bias.stride())
    return bias


def _per_image_f32(t, B, name, expand=False):
    """None, or `t` as the contiguous fp32 [B] vector the kernels read; expand: a single element serves every image."""
    if t is None:
        return None
    t = t.to(torch.float32).reshape(-1).contiguous()
    if expand and t.numel() == 1 and B > 1:
        t = t.expand(B).contiguous()
    if t.numel() != B:
        raise PwwHipError("%s must have B=%d elements" % (name, B))
    return t


def _check_f64(t, name, *shape):
    """`t` is None or a contiguous float64 tensor of `shape` = (B, ...); an extent given as a string is free and named by it."""
    if t is not None and (t.dtype != torch.float64 or t.dim() != len(shape) or not t.is_contiguous()
                          or any(not isinstance(s, str) and s != n for s, n in zip(shape, t.shape))):
        raise PwwHipError("%s must be a contiguous float64 [%s] tensor" % (name, ", ".join(["B"] + [str(s) for s in shape[1:]])))


def _attention_route(has_bias, stat, scratch, parts, M):
    """The launch attention() takes, decided from which arguments are given and the key count alone (no tensor is touched)."""
    if not has_bias:
        return "self"       # pww_self_attn_fwd
    if stat is None:
        return "plain"      # pww_cross_attn_fwd: c[b] = bias_coeff[b]
    if stat[0] is not None:
        return "stat"       # pww_cross_attn_fwd_stat_ex: the [B, 4] statistics of qk_stats come with the call
    if stat[1] == STAT_NONE and parts is None and M > FUSED_MAX_KEYS:
        return "stat"       # ... with null stats: nothing to form or fold, and only this launch has no key limit (scratch or not)
    # stat = (None, kind, scalar): partials folded at entry (pww_cross_attn_fwd_parts), or, with a FusedScratch, the statistic formed in
    # the launch (pww_cross_attn_fwd_fused_ex, experiments library)
    return "parts" if scratch is None else "fused"


def attention_route(has_bias, stat, scratch, parts, M):
    """The launch attention() takes for these arguments and M keys: _attention_route's table, then by key count alone "long" -- the pair of
    launches of libpww_hip_long.so, which holds the parts contract over FUSED_MAX_KEYS < M <= LONG_MAX_KEYS."""
    route = _attention_route(has_bias, stat, scratch, parts, M)
    if route in ("parts", "stat") and stat[0] is None and scratch is None and long_keys(M):
        return "long"
    return route


def _launch_stat(lib, io, bias, coeff, d, stat, coeff_dev):
    """c[b] = scalar * stat(stats[b]) * coeff[b]; null stats (STAT_NONE): the scalar -- or the hipGraph mode's device word -- alone."""
    stats, kind, scalar = stat
    _check_f64(stats, "stat: stats", d.B, 4)
    op = _cross_opts(d.B, d.N, coeff_dev, 0, None)
    _lib.check(lib.pww_cross_attn_fwd_stat_ex(*io, _ptr(bias), _ptr(stats), int(kind), float(d.H * d.N * d.M), float(scalar), _ptr(coeff),
                                              ctypes.byref(d), _opt_ref(op), _stream()), "pww_cross_attn_fwd_stat_ex")


def _parts_stat(d, stat, parts, missing):
    """(kind, scalar) of stat = (None, kind, scalar) for a launch that folds `parts`: a statistic without its partials raises `missing`."""
    _, kind, scalar = stat
    if kind != STAT_NONE and parts is None:
        raise PwwHipError(missing)
    _check_f64(parts, "parts", d.B, "nparts", 4)
    return kind, scalar


def _parts_args(io, bias, coeff, d, kind, scalar, parts, stats_out, op):
    """The arguments pww_cross_attn_fwd_parts and pww_long_cross_attn_fwd_parts share."""
    return (*io, _ptr(bias), int(kind), float(scalar), _ptr(coeff), ctypes.byref(d), _ptr(parts), int(parts.shape[1]) if parts is not None else 0,
            _ptr(stats_out), _opt_ref(op), _stream())


def _launch_parts(lib, io, bias, coeff, d, stat, parts, stats_out, coeff_dev, bias_cols, compact, gated):
    """Pass 2 only: the statistic's partials came from qproj_stat / qk_parts (none needed for STAT_NONE); nothing in it waits for another workgroup."""
    kind, scalar = _parts_stat(d, stat, parts, "a statistic formed outside the attention launch needs its partials (qproj_stat / qk_parts), or a "
                                               "FusedScratch for the in-launch form")
    if d.M > FUSED_MAX_KEYS:
        raise PwwHipError("the pass-2-only cross-attention launch takes at most %d keys (partials over more keys: fold them with "
                          "fold_parts and pass stat=(stats, kind, scalar))" % FUSED_MAX_KEYS)
    _check_f64(stats_out, "stats_out", d.B, 4)
    if compact is not None and (compact[0].shape[-1] > COMPACT_MAX_R or not _lib.has_experiments()):
        compact = None          # (the compact form of the map is an experiments-library form: the dense map serves)
    op = _cross_opts(d.B, d.N, coeff_dev, bias_cols, compact, gated)
    _lib.check(lib.pww_cross_attn_fwd_parts(*_parts_args(io, bias, coeff, d, kind, scalar, parts, stats_out, op)), "pww_cross_attn_fwd_parts")


def long_keys(M):
    """True for the key counts libpww_hip_long.so serves: prompts encoded in 2 or 3 chunks of 77 tokens (any FUSED_MAX_KEYS < M <= LONG_MAX_KEYS)."""
    return FUSED_MAX_KEYS < M <= LONG_MAX_KEYS


def _launch_long(io, bias, coeff, d, stat, parts, stats_out, coeff_dev, bias_cols, gated):
    """_launch_parts for FUSED_MAX_KEYS < M <= LONG_MAX_KEYS: pww_long_cross_attn_fwd_parts (partials from long_qk_parts; none for STAT_NONE).
    The compact form of the map belongs to the <= 128-key kernel of the experiments library: ops.attention does not hand it on, the dense map serves."""
    kind, scalar = _parts_stat(d, stat, parts, "a statistic over %d keys needs its partials (long_qk_parts)" % d.M)
    _check_f64(stats_out, "stats_out", d.B, 4)
    op = _cross_opts(d.B, d.N, coeff_dev, bias_cols, None, gated)
    lib = _lib.load_long()
    # partials over more than FUSED_MAX_KEYS keys have one producer, and its count is a function of the problem: anything else (partials of
    # qproj_stat / qk_parts, which stop at 128 keys; another layer's) does not describe this Q K^T
    want = int(lib.pww_long_qk_parts_count(ctypes.byref(d))) if parts is not None else 0
    if parts is not None and parts.shape[1] != want:
        raise PwwHipError("cross-attention over %d keys folds the partials of long_qk_parts (%d per image for this problem), got %d: the pass-2-only "
                          "launch of libpww_hip.so takes at most %d keys" % (d.M, want, parts.shape[1], FUSED_MAX_KEYS))
    _lib.check(lib.pww_long_cross_attn_fwd_parts(*_parts_args(io, bias, coeff, d, kind, scalar, parts, stats_out, op)),
               "pww_long_cross_attn_fwd_parts", lib)


def _launch_fused(io, bias, coeff, d, stat, scratch, device, stats_out, coeff_dev, bias_cols, compact, gated):
    """The statistic formed in the attention launch itself, through the workgroup hand-off in `scratch`: not part of the product library."""
    _, kind, scalar = stat
    if d.M > FUSED_MAX_KEYS:
        raise PwwHipError("fused statistic needs a FusedScratch and at most %d keys" % FUSED_MAX_KEYS)
    xlib = _lib.load_experiments()
    state, ws = scratch.ensure(xlib, d, device)
    _check_f64(stats_out, "stats_out", d.B, 4)
    if compact is not None and compact[0].shape[-1] > COMPACT_MAX_R:
        compact = None
    op = _cross_opts(d.B, d.N, coeff_dev, bias_cols, compact, gated)
    _lib.check(xlib.pww_cross_attn_fwd_fused_ex(*io, _ptr(bias), int(kind), float(scalar), _ptr(coeff), ctypes.byref(d), _ptr(stats_out), _ptr(state),
                                                state.numel() * 8, _ptr(ws), ws.numel() * 8, _opt_ref(op), _stream()), "pww_cross_attn_fwd_fused_ex", xlib)


def attention(q, k, v, heads, scale, bias=None, bias_coeff=None, stat=None, scratch=None, stats_out=None, coeff_dev=None,
              bias_cols=0, compact=None, gated=0, parts=None):
    """softmax((Q K^T + c * bias) * scale) V on [B, tokens, heads*D] tensors (diffusers layout, no
    head-split copies). bias: fp32 tensor broadcastable to [B, heads, N, M] or None;
    bias_coeff: optional fp32 [B] device tensor of per-image coefficients (with `stat`: the row gate);
    stat: optional (stats, STAT_* kind, python scalar): the kernel forms c[b] = scalar * stat(stats[b]) * bias_coeff[b]
    itself. `stats` is either the float64 [B,4] tensor of qk_stats (pww_cross_attn_fwd_stat) or None together with a
    FusedScratch in `scratch`: the statistic is then computed in the same launch (pww_cross_attn_fwd_fused, M <= 128).
    With `stat`: coeff_dev = one-element fp32 device tensor that replaces the python scalar when the kernel runs (hipGraph
    replays across denoise steps); bias_cols = columns >= bias_cols of the map are zero; compact = (values [B?, N, R] fp32,
    col_idx [B?, R] int32) the compact form of the same map (fused launch only); gated = the caller's hint that bias_coeff is
    non-zero exactly for the first `gated` images (a CFG-folded batch), 0 = unknown (fused launch only: work distribution).
    parts: float64 [B, nparts, 4] partials of the statistic formed by qproj_stat with q (stat = (None, kind, scalar)): the launch
    folds them at entry (pww_cross_attn_fwd_parts) -- no scratch, no hand-off."""
    _require_gpu(q, k, v, bias, bias_coeff)
    if not (q.dtype == k.dtype == v.dtype):
        raise PwwHipError("q/k/v dtypes differ: %s %s %s" % (q.dtype, k.dtype, v.dtype))
    q, k, v = _prep(q), _prep(k), _prep(v)
    B, N, C = q.shape
    out = torch.empty((B, N, C), dtype=q.dtype, device=q.device)
    d = _desc(q, k, v, out, heads, scale)
    lib = _lib.load()
    route = attention_route(bias is not None, stat, scratch, parts, d.M)
    io = (_ptr(q), _ptr(k), _ptr(v), _ptr(out))
    if route != "self":
        bias = _bias_view(bias, d)
        bias_coeff = _per_image_f32(bias_coeff, B, "bias_coeff", expand=True)
    with torch.cuda.device(q.device):
        if route == "self":
            _lib.check(lib.pww_self_attn_fwd(*io, ctypes.byref(d), _stream()), "pww_self_attn_fwd")
        elif route == "plain":
            _lib.check(lib.pww_cross_attn_fwd(*io, _ptr(bias), _ptr(bias_coeff), ctypes.byref(d), _stream()), "pww_cross_attn_fwd")
        elif route == "stat":
            _launch_stat(lib, io, bias, bias_coeff, d, stat, coeff_dev)
        elif route == "parts":
            _launch_parts(lib, io, bias, bias_coeff, d, stat, parts, stats_out, coeff_dev, bias_cols, compact, gated)
        elif route == "long":
            _launch_long(io, bias, bias_coeff, d, stat, parts, stats_out, coeff_dev, bias_cols, gated)
        else:
            _launch_fused(io, bias, bias_coeff, d, stat, scratch, q.device, stats_out, coeff_dev, bias_cols, compact, gated)
    return out


def probs_buffer(images, N, M, device, zero=True):
    """An fp32 [images, N, M] tensor attention_probs can write to: rows of M floats in storage padded to a multiple of 4 (16-byte aligned rows)."""
    make = torch.zeros if zero else torch.empty
    return make((images, N, (M + 3) & ~3), dtype=torch.float32, device=device)[:, :, :M]


def attention_probs(q, k, heads, scale, bias=None, bias_coeff=None, stat=None, coeff_dev=None, images=0, out=None, accumulate=False, weight=1.0):
    """weight * mean over heads of softmax((Q K^T + c * bias) * scale): the fp32 [images, N, M] probabilities the attention launch of the same
    arguments keeps in registers (reference: `attention_scores.softmax(dim=-1)`, paint_with_words.py:112-114), from a launch of its own
    (pww_cross_attn_probs, M <= 128). q, k, bias, bias_coeff and coeff_dev mean what they mean in `attention`; stat = (stats, kind, scalar) with
    `stats` the float64 [B, 4] tensor of qk_stats -- or the `stats_out` a parts-route attention launch wrote -- and None only with STAT_NONE:
    c[b] = scalar * stat(stats[b]) * bias_coeff[b]. Without `stat`: c[b] = bias_coeff[b]. images: only the first so many images are computed
    (0 = all; a CFG-folded batch is [cond rows; uncond rows]). out: an fp32 [>= images, N, >= M] tensor to write to (unit stride along the keys, row
    and image strides multiples of 4) -- with accumulate, to add to; returned as given."""
    _require_gpu(q, k, bias, bias_coeff, out)
    if q.dtype != k.dtype:
        raise PwwHipError("q/k dtypes differ: %s %s" % (q.dtype, k.dtype))
    q, k = _prep(q), _prep(k)
    d = _desc(q, k, None, None, heads, scale)
    B, N, M = d.B, d.N, d.M
    if M > LONG_MAX_KEYS:
        raise PwwHipError("attention_probs takes at most %d keys (got %d)" % (LONG_MAX_KEYS, M))
    n_img = int(images or 0)
    if n_img < 0 or n_img > B:
        raise PwwHipError("attention_probs: images = %d outside 0 .. B = %d" % (n_img, B))
    rows = n_img or B
    if bias is not None:
        bias = _bias_view(bias, d)
        bias_coeff = _per_image_f32(bias_coeff, B, "bias_coeff", expand=True)
    else:
        bias_coeff = None
    stats, kind, scalar = stat if stat is not None else (None, STAT_NONE, 1.0)
    _check_f64(stats, "stat: stats", B, 4)
    if stats is None and kind != STAT_NONE:
        raise PwwHipError("attention_probs: a statistic needs its [B, 4] statistics (qk_stats, or the stats_out of the attention launch)")
    if out is None:
        if accumulate:
            raise PwwHipError("attention_probs: accumulate needs `out`")
        out = probs_buffer(rows, N, M, q.device, zero=False)
    elif (out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] < rows or out.shape[1] != N or out.shape[2] < M or out.stride(2) != 1
          or out.stride(1) % 4 or out.stride(0) % 4 or out.data_ptr() % 16 or out.device != q.device):
        raise PwwHipError("attention_probs: `out` must be an fp32 [>= %d, %d, >= %d] tensor on %s, 16-byte aligned, unit key stride, row / image strides "
                          "multiples of 4" % (rows, N, M, q.device))
    pd = ProbsDesc(ctypes.sizeof(ProbsDesc), n_img, int(bool(accumulate)), float(weight))
    pd.out_stride[:] = [out.stride(0), out.stride(1)]
    op = _cross_opts(B, N, coeff_dev, 0, None)
    lib = _lib.load_long() if long_keys(M) else _lib.load()
    launch, name = (lib.pww_long_cross_attn_probs, "pww_long_cross_attn_probs") if long_keys(M) else (lib.pww_cross_attn_probs, "pww_cross_attn_probs")
    with torch.cuda.device(q.device):
        _lib.check(launch(_ptr(q), _ptr(k), _ptr(bias), _ptr(stats), int(kind), float(d.H * N * M), float(scalar), _ptr(bias_coeff),
                          ctypes.byref(d), _opt_ref(op), _ptr(out), ctypes.byref(pd), _stream()), name, lib)
    return out


def attention_out_supported(q, k, heads, bias, weight, bias_cols=0):
    """EXPERIMENTS LIBRARY. True if attention_out (cross-attention + to_out in one launch) takes this problem: C = heads * D = 320 with D <= 64, 64 <= M <= 128,
    a dense fp32 map shared by the heads with at most 64 non-zero columns, weight [C, C] of q's dtype."""
    if q.dtype not in _DT or q.dim() != 3 or k.dim() != 3 or bias is None or not torch.is_tensor(weight):
        return False
    B, N, C = q.shape
    M = k.shape[1]
    if tuple(weight.shape) != (C, C) or weight.dtype != q.dtype or not weight.is_contiguous() or C % heads:
        return False
    d = AttnDesc()
    d.dtype = _DT[q.dtype]
    d.B, d.H, d.N, d.M, d.D = B, heads, N, M, C // heads
    d.q_stride[:] = [q.stride(0), C // heads, q.stride(1)]
    try:
        _bias_view(bias, d)
    except RuntimeError:
        return False
    return bool(_lib.load_experiments().pww_cross_attn_out_supported(ctypes.byref(d), C, int(bias_cols)))


def attention_out(q, k, v, heads, scale, bias, weight, weight_bias=None, residual=None, bias_coeff=None, stat=None, parts=None, stats_out=None,
                  coeff_dev=None, bias_cols=0, gated=0):
    """EXPERIMENTS LIBRARY (libpww_hip_experiments.so: measured slower than the two-launch route at batch 1, a tie at 16 rows --
    profiles/r05_to_out_epilogue.md; not a product route since round 6).
    linear(attention(q, k, v, ...), weight, weight_bias) [+ residual] in ONE launch (pww_cross_attn_fwd_parts_out: reference
    paint_with_words.py:106-123): the pass-2-only cross-attention of `attention(..., stat=(None, kind, scalar), parts=parts)` with the
    layer's to_out projection applied to the heads' outputs while they are still in registers. stat = (None, kind, scalar) or None
    (= a plain `bias_coeff * bias`). Ask attention_out_supported first; anything else raises."""
    _require_gpu(q, k, v, bias, bias_coeff, weight, weight_bias, residual)
    if not (q.dtype == k.dtype == v.dtype == weight.dtype):
        raise PwwHipError("q/k/v/weight dtypes differ: %s %s %s %s" % (q.dtype, k.dtype, v.dtype, weight.dtype))
    q, k, v = _prep(q), _prep(k), _prep(v)
    B, N, C = q.shape
    if tuple(weight.shape) != (C, C) or not weight.is_contiguous():
        raise PwwHipError("attention_out: weight must be a contiguous [%d, %d] tensor" % (C, C))
    if weight_bias is not None and (weight_bias.dtype != q.dtype or tuple(weight_bias.shape) != (C,) or not weight_bias.is_contiguous()):
        raise PwwHipError("attention_out: weight_bias must be a contiguous [%d] tensor of q's dtype" % C)
    if residual is not None and (residual.dtype != q.dtype or tuple(residual.shape) != (B, N, C) or residual.stride(2) != 1):
        raise PwwHipError("attention_out: residual must be a [B, N, C] tensor of q's dtype with unit channel stride")
    out = torch.empty((B, N, C), dtype=q.dtype, device=q.device)
    d = _desc(q, k, v, out, heads, scale)
    bias = _bias_view(bias, d)
    bias_coeff = _per_image_f32(bias_coeff, B, "bias_coeff", expand=True)
    if stat is not None and stat[0] is not None:
        raise PwwHipError("attention_out folds partials (stat = (None, kind, scalar), parts = qproj_stat / qk_parts output)")
    kind, scalar = _parts_stat(d, stat or (None, STAT_NONE, 1.0), parts, "attention_out: a statistic needs its partials (qproj_stat / qk_parts)")
    _check_f64(stats_out, "stats_out", B, 4)
    op = _cross_opts(B, N, coeff_dev, bias_cols, None, gated)
    rs = (ctypes.c_int64 * 2)(residual.stride(0), residual.stride(1)) if residual is not None else None
    lib = _lib.load_experiments()
    with torch.cuda.device(q.device):
        rc = lib.pww_cross_attn_fwd_parts_out(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(bias), int(kind), float(scalar), _ptr(bias_coeff), ctypes.byref(d),
                                              _ptr(parts), int(parts.shape[1]) if parts is not None else 0, _ptr(stats_out),
                                              _opt_ref(op), _ptr(weight), _ptr(weight_bias), _ptr(residual), rs, _stream())
    _lib.check(rc, "pww_cross_attn_fwd_parts_out", lib)
    return out


def _qproj_desc(x, weight, k, heads):
    if x.dim() != 3 or k.dim() != 3 or weight.dim() != 2:
        raise PwwHipError("qproj: x [B, N, Cin], weight [C, Cin], k [B or 1, M, C]")
    B, N, Cin = x.shape
    C = weight.shape[0]
    if weight.shape[1] != Cin or k.shape[2] != C or k.shape[0] not in (1, B) or C % heads:
        raise PwwHipError("qproj: shapes do not fit (x %s, weight %s, k %s, heads %d)" % (tuple(x.shape), tuple(weight.shape), tuple(k.shape), heads))
    d = QprojDesc()
    d.dtype = _DT[x.dtype]
    d.B, d.N, d.Cin, d.H, d.D, d.M = B, N, Cin, heads, C // heads, k.shape[1]
    d.x_stride[:] = [x.stride(0), x.stride(1)]
    d.k_stride[:] = [k.stride(0) if k.shape[0] == B and B > 1 else 0, k.stride(1)]
    return d


def qproj_parts(x, weight, k, heads):
    """Partials per image pww_qproj_stat forms for this problem, 0 if the shape is not supported (the caller then keeps its own
    projection and the in-launch statistic)."""
    if x.dtype not in _DT or not (x.dtype == weight.dtype == k.dtype) or k.shape[1] > FUSED_MAX_KEYS:
        return 0
    d = _qproj_desc(x, weight, k, heads)
    d.q_stride[:] = [x.shape[1] * weight.shape[0], weight.shape[0]]
    return int(_lib.load().pww_qproj_parts(ctypes.byref(d)))


def qproj_stat(x, weight, k, heads, kind, gate=None):
    """q = x @ weight.T (a bias-free to_q, paint_with_words.py:76) together with the partials of the per-image score statistic
    of q k^T (:87; kind = STAT_*: only the fields that statistic needs are formed) -- one launch, the statistic comes out of the GEMM's
    epilogue. Returns (q [B, N, C], parts float64 [B, nparts, 4]). gate: optional fp32 [B]; images with gate 0 get no partials."""
    _require_gpu(x, weight, k, gate)
    if not (x.dtype == weight.dtype == k.dtype):
        raise PwwHipError("qproj: dtypes differ: %s %s %s" % (x.dtype, weight.dtype, k.dtype))
    x, k = _prep(x), _prep(k)
    weight = weight if weight.is_contiguous() else weight.contiguous()
    B, N, Cin = x.shape
    C = weight.shape[0]
    q = torch.empty((B, N, C), dtype=x.dtype, device=x.device)
    d = _qproj_desc(x, weight, k, heads)
    d.q_stride[:] = [q.stride(0), q.stride(1)]
    lib = _lib.load()
    nparts = int(lib.pww_qproj_parts(ctypes.byref(d)))
    if nparts <= 0:
        raise PwwHipError("qproj_stat: unsupported shape (C = %d, head dim %d, Cin = %d): ask qproj_parts() first" % (C, C // heads, Cin))
    parts = torch.empty((B, nparts, 4), dtype=torch.float64, device=x.device)
    gate = _per_image_f32(gate, B, "gate")
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_qproj_stat(_ptr(x), _ptr(weight), _ptr(q), _ptr(k), _ptr(gate), ctypes.byref(d), int(kind), _ptr(parts),
                                      parts.numel() * 8, _stream()), "pww_qproj_stat")
    return q, parts


def _stat_parts(name, load, q, k, heads, kind, gate, gated=0, per_head=False):
    """The body of qk_parts, long_qk_parts and scope_head_parts (`name`): the library `load()` returns holds the launch pww_<name> and its
    count query pww_<name>_count. per_head: partials per (image, head) -- [B, heads, nparts, 4] -- and a launch without the `gated` hint."""
    _require_gpu(q, k, gate)
    if q.dtype != k.dtype:
        raise PwwHipError("%s: dtypes differ: %s %s" % (name, q.dtype, k.dtype))
    q, k = _prep(q), _prep(k)
    d = _desc(q, k, None, None, heads, 1.0)
    lib = load()
    nparts = int(getattr(lib, "pww_%s_count" % name)(ctypes.byref(d)))
    if nparts <= 0:
        raise PwwHipError("%s: unsupported problem %s x %s, %d heads" % (name, tuple(q.shape), tuple(k.shape), heads))
    B = q.shape[0]
    parts = torch.empty((B, heads, nparts, 4) if per_head else (B, nparts, 4), dtype=torch.float64, device=q.device)
    gate = _per_image_f32(gate, B, "gate")
    hint = () if per_head else (int(gated or 0),)
    with torch.cuda.device(q.device):
        _lib.check(getattr(lib, "pww_" + name)(_ptr(q), _ptr(k), _ptr(gate), ctypes.byref(d), int(kind), *hint, _ptr(parts), parts.numel() * 8, _stream()),
                   "pww_" + name, lib)
    return parts


def qk_parts(q, k, heads, kind, gate=None, gated=0):
    """Partials of the per-image score statistic of q k^T over a FINISHED q (paint_with_words.py:87 + the reduction weight_function
    applies): float64 [B, nparts, 4], the input of attention(..., parts=...). One small launch (pww_qk_parts): the layers whose to_q
    stays the stock GEMM. gate: optional fp32 [B] (images with gate 0 get no partials); gated: hint that exactly the first `gated`
    images have a non-zero gate."""
    return _stat_parts("qk_parts", _lib.load, q, k, heads, kind, gate, gated)


def long_qk_parts(q, k, heads, kind, gate=None, gated=0):
    """qk_parts for FUSED_MAX_KEYS < M <= LONG_MAX_KEYS (pww_long_qk_parts): float64 [B, nparts, 4], the input of attention(..., parts=...)."""
    return _stat_parts("long_qk_parts", _lib.load_long, q, k, heads, kind, gate, gated)


SCOPE_HEAD, SCOPE_ROW = _lib.SCOPE_HEAD, _lib.SCOPE_ROW   # PWW_SCOPE_* of include/pww_hip_scope.h
_SCOPED_KINDS = (STAT_MAX, STAT_MIN, STAT_MEAN, STAT_STD, STAT_ABSMAX)


def scoped_available():
    """True if libpww_hip_scope.so is there (a stale or broken file raises, with the rebuild hint)."""
    return _lib.load_scope() is not None


def _scope_lib():
    lib = _lib.load_scope()
    if lib is None:
        raise PwwHipError("libpww_hip_scope.so not found at %s: per-head / per-row score statistics need it. Build it with "
                          "`python paint-with-words-sd_amd/build.py` (or __graft_entry__.build())." % _lib.SCOPE_LIB_PATH)
    return lib


def scope_head_parts(q, k, heads, kind, gate=None):
    """Partials of the score statistic of q k^T PER (image, head) over a finished q: float64 [B, heads, nparts, 4] = (max, min, sum, sum of
    squares), the input of attention_scoped(..., scope=SCOPE_HEAD, parts=...). One small launch (pww_scope_head_parts, M <= 128).
    gate: optional fp32 [B]; images with gate 0 get no partials (their rows are left as allocated)."""
    return _stat_parts("scope_head_parts", _scope_lib, q, k, heads, kind, gate, per_head=True)


def attention_scoped(q, k, v, heads, scale, bias, kind, scope, scalar, gate=None, parts=None, stats_out=None, coeff_dev=None):
    """softmax((Q K^T + c * bias) * scale) V on [B, tokens, heads*D] tensors with the coefficient a statistic of the raw scores per head
    (scope = SCOPE_HEAD: c[b][h] = scalar * stat(scores of image b, head h) * gate[b], folded from `parts` = scope_head_parts(q, k, ...))
    or per query row (SCOPE_ROW: c[b][h][n] = scalar * stat(scores of that row) * gate[b], formed in registers: no partials).
    bias: fp32 tensor broadcastable to [B, heads, N, M] with unit key stride; kind: STAT_MAX / MIN / MEAN / STD / ABSMAX; gate: optional
    fp32 [B] per-image factor (0 = no bias for that image); coeff_dev: one-element fp32 device tensor that replaces `scalar` when the
    kernel runs; stats_out (head scope): float64 [B, heads, 4] that receives the folded fields. M <= 128 (pww_scope_cross_attn_fwd)."""
    _require_gpu(q, k, v, bias, gate, parts, stats_out)
    if not (q.dtype == k.dtype == v.dtype):
        raise PwwHipError("q/k/v dtypes differ: %s %s %s" % (q.dtype, k.dtype, v.dtype))
    if bias is None:
        raise PwwHipError("attention_scoped needs a bias map")
    if scope not in (SCOPE_HEAD, SCOPE_ROW) or kind not in _SCOPED_KINDS:
        raise PwwHipError("attention_scoped: scope %r / statistic %r outside SCOPE_HEAD, SCOPE_ROW / STAT_MAX ... STAT_ABSMAX" % (scope, kind))
    q, k, v = _prep(q), _prep(k), _prep(v)
    B, N, C = q.shape
    out = torch.empty((B, N, C), dtype=q.dtype, device=q.device)
    d = _desc(q, k, v, out, heads, scale)
    if d.M > FUSED_MAX_KEYS:
        raise PwwHipError("attention_scoped takes at most %d keys (got %d)" % (FUSED_MAX_KEYS, d.M))
    bias = _bias_view(bias, d)
    gate = _per_image_f32(gate, B, "gate", expand=True)
    if scope == SCOPE_HEAD:
        if parts is None:
            raise PwwHipError("attention_scoped: head scope folds the partials of scope_head_parts")
        _check_f64(parts, "parts", B, heads, "nparts", 4)
        _check_f64(stats_out, "stats_out", B, heads, 4)
    elif parts is not None or stats_out is not None:
        raise PwwHipError("attention_scoped: row scope takes no partials and writes no stats_out")
    op = _cross_opts(B, N, coeff_dev, 0, None)
    lib = _scope_lib()
    with torch.cuda.device(q.device):
        _lib.check(lib.pww_scope_cross_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(bias), int(kind), int(scope), float(scalar), _ptr(gate),
                                                ctypes.byref(d), _ptr(parts), int(parts.shape[2]) if parts is not None else 0, _ptr(stats_out),
                                                _opt_ref(op), _stream()), "pww_scope_cross_attn_fwd", lib)
    return out


def fold_parts(parts):
    """[B, nparts, 4] partials -> [B, 4] statistics (max, min, sum, sum of squares), as the attention kernel folds them."""
    return torch.stack([parts[:, :, 0].amax(1), parts[:, :, 1].amin(1), parts[:, :, 2].sum(1), parts[:, :, 3].sum(1)], dim=1)


def qk_stats(q, k, heads):
    """Per-image statistics of the raw scores Q K^T over heads x rows x keys: float64 [B, 4] =
    (max, min, sum, sum of squares). q: [B, N, heads*D], k: [B, M, heads*D]."""
    _require_gpu(q, k)
    q, k = _prep(q), _prep(k)
    stats = torch.empty((q.shape[0], 4), dtype=torch.float64, device=q.device)
    d = _desc(q, k, None, None, heads, 1.0)
    lib = _lib.load()
    nbytes = int(lib.pww_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=q.device)   # caching allocator: stream-ordered reuse
    with torch.cuda.device(q.device):
        _lib.check(lib.pww_qk_reduce(_ptr(q), _ptr(k), ctypes.byref(d), _ptr(stats), _ptr(ws), ws.numel() * 8, _stream()),
                   "pww_qk_reduce")
    return stats


def _regions_tensor(regions, device):
    """[(r, g, b, strength)] -> device byte tensor laid out as struct pww_region[R]."""
    arr = (Region * len(regions))()
    for i, (r, g, b, s) in enumerate(regions):
        arr[i] = Region(int(r), int(g), int(b), 0, float(s))
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return raw.to(device)


def _csr(cols, device):
    ptr, reg = [0], []
    for lst in cols:
        reg.extend(int(x) for x in lst)
        ptr.append(len(reg))
    col_ptr = torch.tensor(ptr, dtype=torch.int32).to(device)
    col_reg = torch.tensor(reg if reg else [0], dtype=torch.int32).to(device)
    return col_ptr, col_reg


def round_half_up_div(a, ratio):
    return (2 * a + ratio) // (2 * ratio)


def _level_rows(H, W, ratios):
    """{ratio: Hr * Wr}. A level without pixels is refused here: its empty output tensor has a null data pointer, which the C entry
    points take for "skip this level", so the library's own refusal would never be reached."""
    rows = {}
    for r in ratios:
        rows[r] = round_half_up_div(H, r) * round_half_up_div(W, r) if r > 0 else 0
        if rows[r] <= 0:
            raise PwwHipError("mask_build: image %dx%d too small for ratio %d" % (H, W, r))
    return rows


def mask_build(rgb, regions, cols, ratios=(8, 16, 32, 64)):
    """RGB color map (uint8 [H, W, 3] device tensor) -> {ratio: fp32 [Hr*Wr, T]} token weight maps.
    regions: [(r, g, b, strength)]; cols: per prompt position, the region ordinals added to it."""
    _require_gpu(rgb)
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise PwwHipError("rgb must be uint8 [H, W, 3]")
    rgb = rgb.contiguous()
    H, W = rgb.shape[:2]
    T = len(cols)
    dev = rgb.device
    rows = _level_rows(H, W, ratios)
    regs = _regions_tensor(regions, dev)
    col_ptr, col_reg = _csr(cols, dev)
    outs = {r: torch.empty((rows[r], T), dtype=torch.float32, device=dev) for r in ratios}
    lib = _lib.load()
    with torch.cuda.device(dev):
        if tuple(ratios) == (8, 16, 32, 64):
            rc = lib.pww_mask_build(_ptr(rgb), H, W, _ptr(regs), len(regions), _ptr(col_ptr), _ptr(col_reg), T,
                                    _ptr(outs[8]), _ptr(outs[16]), _ptr(outs[32]), _ptr(outs[64]), _stream())
            _lib.check(rc, "pww_mask_build")
        else:
            for r in ratios:
                rc = lib.pww_mask_build_rgb(_ptr(rgb), H, W, _ptr(regs), len(regions), _ptr(col_ptr), _ptr(col_reg),
                                            T, r, _ptr(outs[r]), _stream())
                _lib.check(rc, "pww_mask_build_rgb")
    return outs


def mask_build_f32(masks, cols, ratios=(8, 16, 32, 64)):
    """Same accumulation from R float32 region masks [R, H, W] (strength-scaled, possibly blurred)."""
    _require_gpu(masks)
    masks = masks.to(torch.float32).contiguous()
    R, H, W = masks.shape
    T = len(cols)
    dev = masks.device
    rows = _level_rows(H, W, ratios)
    col_ptr, col_reg = _csr(cols, dev)
    outs = {}
    lib = _lib.load()
    with torch.cuda.device(dev):
        for r in ratios:
            outs[r] = torch.empty((rows[r], T), dtype=torch.float32, device=dev)
        rest = list(ratios)
        if all(r in outs for r in (8, 16, 32, 64)):       # the four maps of a request: ONE launch
            rc = lib.pww_mask_build_f32_levels(_ptr(masks), H, W, R, _ptr(col_ptr), _ptr(col_reg), T, _ptr(outs[8]), _ptr(outs[16]),
                                               _ptr(outs[32]), _ptr(outs[64]), _stream())
            _lib.check(rc, "pww_mask_build_f32_levels")
            rest = [r for r in ratios if r not in (8, 16, 32, 64)]
        for r in rest:
            rc = lib.pww_mask_build_f32(_ptr(masks), H, W, R, _ptr(col_ptr), _ptr(col_reg), T, r, _ptr(outs[r]), _stream())
            _lib.check(rc, "pww_mask_build_f32")
    return outs


def resize_tokens(w_orig, n_tokens):
    """CROSS_ATTENTION_WEIGHT_ORIG [H, W, T] (fp32, device) -> [n_tokens, T]: the reference's fallback resize
    (paint_with_words.py:96-101). The intermediate size is computed like torch does for `scale_factor`."""
    import math
    _require_gpu(w_orig)
    if w_orig.dim() != 3 or w_orig.dtype != torch.float32:
        raise PwwHipError("resize_tokens needs an fp32 [H, W, T] map")
    w_orig = w_orig.contiguous()
    H, W, T = w_orig.shape
    ratio = math.sqrt(H * W / n_tokens)
    oh, ow = int(math.floor(H * (1 / ratio))), int(math.floor(W * (1 / ratio)))
    out = torch.empty((n_tokens, T), dtype=torch.float32, device=w_orig.device)
    with torch.cuda.device(w_orig.device):
        _lib.check(_lib.load().pww_resize_tokens(_ptr(w_orig), H, W, T, oh, ow, int(n_tokens), _ptr(out), _stream()), "pww_resize_tokens")
    return out


def gaussian_kernel1d(sigma, ksize=39):
    """torchvision's _get_gaussian_kernel1d in fp32: exp(-0.5 (x / sigma)^2) on linspace(-h, h, ksize), normalised."""
    half = (ksize - 1) * 0.5
    x = torch.linspace(-half, half, steps=ksize, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gauss_blur(mask, sigma, ksize=39):
    """GaussianBlur(ksize x ksize, sigma) with reflect padding of one fp32 [H, W] device mask (paint_with_words.py:307-312)."""
    _require_gpu(mask)
    if mask.dim() != 2:
        raise PwwHipError("gauss_blur needs an [H, W] mask")
    mask = mask.to(torch.float32).contiguous()
    H, W = mask.shape
    k = gaussian_kernel1d(float(sigma), ksize).to(mask.device)
    tmp = torch.empty((H, W), dtype=torch.float64, device=mask.device)
    out = torch.empty_like(mask)
    with torch.cuda.device(mask.device):
        _lib.check(_lib.load().pww_gauss_blur(_ptr(mask), _ptr(out), H, W, _ptr(k), int(ksize), _ptr(tmp), _stream()), "pww_gauss_blur")
    return out


def inpaint_prep(rgb, mask, lat_h, lat_w):
    """uint8 init image [H, W, 3] + uint8 mask [H, W] (device) -> (mask [1,1,H,W], masked_image [1,3,H,W], latent-size
    mask [1,1,h,w]) fp32, as paint_with_words_inpaint.py:92-106 / :115 compute them."""
    _require_gpu(rgb, mask)
    if rgb.dtype != torch.uint8 or mask.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3 or tuple(mask.shape) != tuple(rgb.shape[:2]):
        raise PwwHipError("inpaint_prep needs uint8 rgb [H, W, 3] and uint8 mask [H, W]")
    rgb, mask = rgb.contiguous(), mask.contiguous()
    H, W = mask.shape
    dev = rgb.device
    m = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
    masked = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
    ml = torch.empty((1, 1, lat_h, lat_w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pww_inpaint_prep(_ptr(rgb), _ptr(mask), H, W, int(lat_h), int(lat_w), _ptr(m), _ptr(masked), _ptr(ml), _stream()),
                   "pww_inpaint_prep")
    return m, masked, ml


def store_f32(dst, values):
    """dst[:len(values)] = values (Python floats, at most 64) as ONE asynchronous launch on the current stream: the values ride
    in the kernel arguments -- no host staging buffer that a later call could overwrite, no synchronous copy."""
    _require_gpu(dst)
    n = len(values)
    if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.numel() < n:
        raise PwwHipError("store_f32 needs a contiguous float32 device tensor with room for %d values" % n)
    arr = (ctypes.c_float * n)(*[float(v) for v in values])
    with torch.cuda.device(dst.device):
        _lib.check(_lib.load().pww_store_f32(_ptr(dst), arr, n, _stream()), "pww_store_f32")


def cfg_combine(cond, uncond, guidance_scale):
    """uncond + g * (cond - uncond) in fp32 (returns fp32)."""
    _require_gpu(cond, uncond)
    if cond.dtype != uncond.dtype or cond.dtype not in _DT or cond.shape != uncond.shape:
        raise PwwHipError("cfg_combine needs two same-shape float16/bfloat16 tensors")
    cond, uncond = cond.contiguous(), uncond.contiguous()
    out = torch.empty(cond.shape, dtype=torch.float32, device=cond.device)
    with torch.cuda.device(cond.device):
        _lib.check(_lib.load().pww_cfg_combine(_ptr(cond), _ptr(uncond), float(guidance_scale), _ptr(out),
                                               cond.numel(), _DT[cond.dtype], _stream()), "pww_cfg_combine")
    return out


# ---- region prompts (libpww_hip_regions.so, include/pww_hip_regions.h) -------------------------------------------------------------------
def region_masks(rgb, colors, feather=0.0):
    """uint8 colour map [H, W, 3] (device) + K (r, g, b) colours -> fp32 [K, H // 8, W // 8]: per latent pixel the share of its 8 x 8 pixel
    block that has colour k exactly, feathered by a Gaussian of sigma `feather` latent pixels if that is > 0. One launch."""
    _require_gpu(rgb)
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise PwwHipError("region_masks needs a uint8 colour map [H, W, 3]")
    rgb = rgb.contiguous()
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    K = len(colors)
    flat = [int(v) for c in colors for v in c]
    if len(flat) != 3 * K or any(not 0 <= v <= 255 for v in flat):
        raise PwwHipError("region_masks needs (r, g, b) colours of 8-bit values")
    host = (ctypes.c_uint8 * max(len(flat), 1))(*flat)
    out = torch.empty((K, H // 8, W // 8), dtype=torch.float32, device=rgb.device)
    lib = _lib.load_regions()
    with torch.cuda.device(rgb.device):
        _lib.check(lib.pww_regions_masks(_ptr(rgb), H, W, host, K, float(feather), _ptr(out), _stream()), "pww_regions_masks", lib)
    return out


def region_combine(eps, masks, weights, scales, guidance_scale):
    """The blend of one step's noise predictions (returns fp32 [n, C, h, w]): eps [(K + 2) n, C, h, w] float16 / bfloat16 with rows
    [base x n, region 1 x n, ..., region K x n, unconditional x n], masks fp32 [n, K, h, w], weights / scales fp32 [n, K]:
    e_u + w_0 g (e_0 - e_u) + sum_k w_k s_k (e_k - e_u) with w_k = weights[k] * masks[k] and w_0 = 1 - sum_k w_k, in fp32, in that order."""
    _require_gpu(eps, masks, weights, scales)
    if eps.dtype not in _DT or eps.dim() != 4 or masks.dim() != 4:
        raise PwwHipError("region_combine needs a float16 / bfloat16 [(K + 2) n, C, h, w] tensor and fp32 masks [n, K, h, w]")
    n, K = int(masks.shape[0]), int(masks.shape[1])
    if (eps.shape[0] != (K + 2) * n or tuple(eps.shape[-2:]) != tuple(masks.shape[-2:]) or tuple(weights.shape) != (n, K) or tuple(scales.shape) != (n, K)
            or any(t.dtype != torch.float32 for t in (masks, weights, scales))):
        raise PwwHipError("region_combine: eps %s does not go with masks %s, weights %s and scales %s (fp32)"
                          % (tuple(eps.shape), tuple(masks.shape), tuple(weights.shape), tuple(scales.shape)))
    eps, masks, weights, scales = eps.contiguous(), masks.contiguous(), weights.contiguous(), scales.contiguous()
    C, h, w = (int(v) for v in eps.shape[1:])
    out = torch.empty((n, C, h, w), dtype=torch.float32, device=eps.device)
    lib = _lib.load_regions()
    with torch.cuda.device(eps.device):
        _lib.check(lib.pww_regions_combine(_ptr(eps), _ptr(masks), _ptr(weights), _ptr(scales), float(guidance_scale), _ptr(out), n, K, C, h * w,
                                           _DT[eps.dtype], _stream()), "pww_regions_combine", lib)
    return out


# ---- canvases larger than the UNet's window (libpww_hip_canvas.so, include/pww_hip_canvas.h) ---------------------------------------------
def canvas_windows(L, win, stride):
    """The window origins along an axis of latent length L: 0, stride, 2 stride, ... below L - win, then L - win (the last window is
    clamped to the end: its origin may be odd and its overlap larger). A tuple of ints."""
    L, win, stride = int(L), int(win), int(stride)
    if win < 1 or L < win or not 1 <= stride <= win:
        raise ValueError("canvas_windows: length %d, window %d, stride %d (1 <= stride <= window <= length)" % (L, win, stride))
    return tuple(range(0, L - win, stride)) + (L - win,)


def _canvas_origins(ys, xs):
    ys, xs = [int(v) for v in ys], [int(v) for v in xs]
    if not ys or not xs:
        raise PwwHipError("canvas: the window origins ys and xs must not be empty")
    return ys, xs, (ctypes.c_int32 * len(ys))(*ys), (ctypes.c_int32 * len(xs))(*xs)


def canvas_gather(canvas, ys, xs, h, w, denom, copies, dtype):
    """The windows of a canvas latent as UNet input rows: canvas fp32 [C, Hc, Wc] (or [1, C, Hc, Wc]) -> `dtype` [copies * ny * nx, C, h, w],
    window iy * nx + ix = canvas[:, ys[iy]:ys[iy] + h, xs[ix]:xs[ix] + w] / denom (one fp32 division, one rounding), the whole set
    repeated `copies` times (the row classes of a folded call). One launch."""
    _require_gpu(canvas)
    if canvas.dim() == 4 and canvas.shape[0] == 1:
        canvas = canvas[0]
    if canvas.dtype != torch.float32 or canvas.dim() != 3:
        raise PwwHipError("canvas_gather needs a float32 canvas [C, Hc, Wc] (or [1, C, Hc, Wc])")
    if dtype not in _DT:
        raise PwwHipError("canvas_gather: the output type must be float16 or bfloat16 (got %s)" % dtype)
    ys, xs, ys_c, xs_c = _canvas_origins(ys, xs)
    canvas = canvas.contiguous()
    C, Hc, Wc = (int(v) for v in canvas.shape)
    out = torch.empty((int(copies) * len(ys) * len(xs), C, int(h), int(w)), dtype=dtype, device=canvas.device)
    lib = _lib.load_canvas()
    with torch.cuda.device(canvas.device):
        _lib.check(lib.pww_canvas_gather(_ptr(canvas), _ptr(out), ys_c, len(ys), xs_c, len(xs), C, Hc, Wc, int(h), int(w), float(denom), int(copies),
                                         _DT[dtype], _stream()), "pww_canvas_gather", lib)
    return out


def canvas_combine(eps, ys, xs, canvas_hw, guidance_scale, ramp=0, masks=None, weights=None, scales=None):
    """The canvas-sized noise prediction of one step (returns fp32 [1, C, Hc, Wc]): eps [(K + 2) n_w, C, h, w] float16 / bfloat16 with rows
    [base x n_w, region 1 x n_w, ..., region K x n_w, unconditional x n_w] for the n_w = ny nx windows at (ys[iy], xs[ix]); per canvas pixel
    the mean of the covering windows' guided predictions, weighted by p = r_h(ly) r_w(lx), r_L(l) = min(min(l, L - 1 - l) + 1, ramp) (1 when
    ramp = 0), in ascending window index. Without region prompts (masks None, K = 0) a window's prediction is e_u + g (e_0 - e_u); with them
    -- masks fp32 [n_w, K, h, w], weights / scales fp32 [n_w, K], one set per window -- it is region_combine's expression. One launch."""
    _require_gpu(eps, masks, weights, scales)
    ys, xs, ys_c, xs_c = _canvas_origins(ys, xs)
    n_w = len(ys) * len(xs)
    if eps.dtype not in _DT or eps.dim() != 4:
        raise PwwHipError("canvas_combine needs a float16 / bfloat16 [(K + 2) n_w, C, h, w] tensor")
    K = 0
    if masks is not None or weights is not None or scales is not None:
        if masks is None or weights is None or scales is None or masks.dim() != 4:
            raise PwwHipError("canvas_combine: region prompts need masks fp32 [n_w, K, h, w] with weights and scales fp32 [n_w, K]")
        K = int(masks.shape[1])
        if (int(masks.shape[0]) != n_w or tuple(eps.shape[-2:]) != tuple(masks.shape[-2:]) or tuple(weights.shape) != (n_w, K) or tuple(scales.shape) != (n_w, K)
                or any(t.dtype != torch.float32 for t in (masks, weights, scales))):
            raise PwwHipError("canvas_combine: eps %s of %d windows does not go with masks %s, weights %s and scales %s (fp32)"
                              % (tuple(eps.shape), n_w, tuple(masks.shape), tuple(weights.shape), tuple(scales.shape)))
        masks, weights, scales = masks.contiguous(), weights.contiguous(), scales.contiguous()
    if eps.shape[0] != (K + 2) * n_w:
        raise PwwHipError("canvas_combine: eps has %d rows for %d windows and %d regions ((K + 2) n_w = %d)" % (eps.shape[0], n_w, K, (K + 2) * n_w))
    eps = eps.contiguous()
    C, h, w = (int(v) for v in eps.shape[1:])
    Hc, Wc = (int(v) for v in canvas_hw)
    out = torch.empty((1, C, Hc, Wc), dtype=torch.float32, device=eps.device)
    lib = _lib.load_canvas()
    with torch.cuda.device(eps.device):
        _lib.check(lib.pww_canvas_combine(_ptr(eps), _ptr(masks), _ptr(weights), _ptr(scales), float(guidance_scale), _ptr(out), ys_c, len(ys), xs_c,
                                          len(xs), K, C, Hc, Wc, h, w, int(ramp), _DT[eps.dtype], _stream()), "pww_canvas_combine", lib)
    return out


# ---- region strength (libpww_hip_hold.so, include/pww_hip_hold.h) ---------------------------------------------------------------------
def hold_strength_map(rgb, colors, strengths, s0, feather=0.0):
    """uint8 colour map [H, W, 3] (device) + K (r, g, b) colours with their strengths + the base strength s0 -> fp32 [H // 8, W // 8]: per
    latent pixel S = ((s0 + m_1 d_1) + m_2 d_2) + ..., m_k the share of its 8 x 8 pixel block that has colour k exactly and d_k =
    fp32(s_k) - fp32(s0) (one fp32 subtraction, formed here), clamped to [0, 1]; feathered by a Gaussian of sigma `feather` latent pixels if
    that is > 0 (two more launches, no limit on the plane)."""
    import numpy as np
    _require_gpu(rgb)
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise PwwHipError("hold_strength_map needs a uint8 colour map [H, W, 3]")
    rgb = rgb.contiguous()
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    K = len(colors)
    flat = [int(v) for c in colors for v in c]
    if len(flat) != 3 * K or any(not 0 <= v <= 255 for v in flat):
        raise PwwHipError("hold_strength_map needs (r, g, b) colours of 8-bit values")
    if len(strengths) != K:
        raise PwwHipError("hold_strength_map: %d strengths for %d colours" % (len(strengths), K))
    base = np.float32(s0)
    deltas = [float(np.float32(s) - base) for s in strengths]
    host_c = (ctypes.c_uint8 * max(len(flat), 1))(*flat)
    host_d = (ctypes.c_float * max(K, 1))(*deltas)
    out = torch.empty((H // 8, W // 8), dtype=torch.float32, device=rgb.device)
    lib = _lib.load_hold()
    with torch.cuda.device(rgb.device):
        _lib.check(lib.pww_hold_strength_map(_ptr(rgb), host_c, host_d, float(base), _ptr(out), H, W, K, _stream()), "pww_hold_strength_map", lib)
        if float(feather) != 0.0:
            tmp = torch.empty_like(out)
            _lib.check(lib.pww_hold_feather(_ptr(out), _ptr(tmp), _ptr(out), H // 8, W // 8, float(feather), _stream()), "pww_hold_feather", lib)
    return out


def hold_feather(plane, sigma):
    """A separable normalised Gaussian of `sigma` pixels over an fp32 plane [h, w] (device), along the rows and then along the columns, in
    global memory (two launches); returns a new plane."""
    _require_gpu(plane)
    if plane.dtype != torch.float32 or plane.dim() != 2:
        raise PwwHipError("hold_feather needs a float32 plane [h, w]")
    plane = plane.contiguous()
    tmp, out = torch.empty_like(plane), torch.empty_like(plane)
    lib = _lib.load_hold()
    with torch.cuda.device(plane.device):
        _lib.check(lib.pww_hold_feather(_ptr(plane), _ptr(tmp), _ptr(out), int(plane.shape[0]), int(plane.shape[1]), float(sigma), _stream()),
                   "pww_hold_feather", lib)
    return out


def hold_apply(x, x0, z, S, theta, a, b):
    """The hold of one step, IN PLACE on x (and returns it): x = (S < theta) ? a x0 + b z : x, with x, x0, z fp32 [n, C, h, w] and S fp32
    [n, h, w], all contiguous (views are taken as they lie: nothing is copied). A select: held pixels are overwritten whatever they held,
    released pixels are not touched. One launch."""
    _require_gpu(x, x0, z, S)
    if any(t.dtype != torch.float32 for t in (x, x0, z, S)):
        raise PwwHipError("hold_apply needs float32 tensors (got %s)" % [str(t.dtype) for t in (x, x0, z, S)])
    if x.dim() < 2 or x0.shape != x.shape or z.shape != x.shape or tuple(S.shape) != (x.shape[0],) + tuple(x.shape[2:]):
        raise PwwHipError("hold_apply: x %s does not go with x0 %s, z %s and S %s ([n, C, ...] three times and [n, ...])"
                          % (tuple(x.shape), tuple(x0.shape), tuple(z.shape), tuple(S.shape)))
    if not all(t.is_contiguous() for t in (x, x0, z, S)):
        raise PwwHipError("hold_apply needs contiguous tensors (x is written in place)")
    if len({t.device for t in (x, x0, z, S)}) != 1:
        raise PwwHipError("hold_apply needs its tensors on one device")
    n, C = int(x.shape[0]), int(x.shape[1])
    hw = x[0, 0].numel()
    lib = _lib.load_hold()
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_hold_apply(_ptr(x), _ptr(x0), _ptr(z), _ptr(S), float(theta), float(a), float(b), n, C, hw, _stream()), "pww_hold_apply", lib)
    return x


# ---- one sampler step as one launch (libpww_hip_step.so, include/pww_hip_step.h) -----------------------------------------------------------
STEP_LAUNCHES = [0]      # launches of the step kernel (pww_hip.steps.stats)


def sched_step(x, row, model, guidance_scale=0.0, h=None, z=None, u=None):
    """One sampler step, IN PLACE on x (and returns it). x fp32 [n, C, h, w] contiguous; row the step's seven numbers (p, r, a, b, c, e, d':
    pww_hip.steps.plan); model the model output -- a (cond, uncond) pair of float16 / bfloat16 tensors of x's shape, combined with
    guidance_scale as uncond + g (cond - uncond), or ONE fp32 tensor of x's shape. h fp32 like x or None: the previous step's q, read if
    c != 0 and overwritten with this step's. z fp32 like x or None: unit noise, read if e != 0. u None, or a float16 / bfloat16 tensor
    [copies * n, C, h, w]: the next UNet input x' / d', every one of the `copies` row classes the same. Tensors are taken as they lie
    (nothing is copied); the arithmetic and its order are the header's. One launch."""
    pair = isinstance(model, (tuple, list))
    m0, m1 = (model[0], model[1]) if pair else (model, None)
    _require_gpu(x, h, z, u, m0, m1)
    row = [float(v) for v in row]
    if len(row) != _lib.STEP_ROW:
        raise PwwHipError("sched_step needs a row of %d numbers (got %d)" % (_lib.STEP_ROW, len(row)))
    if x.dtype != torch.float32 or any(t is not None and (t.dtype != torch.float32 or t.shape != x.shape) for t in (h, z)):
        raise PwwHipError("sched_step needs float32 x, h and z of one shape")
    if pair:
        if m0.dtype not in _DT or m1.dtype != m0.dtype or m0.shape != x.shape or m1.shape != x.shape:
            raise PwwHipError("sched_step: the cond / uncond pair must be two float16 / bfloat16 tensors of x's shape %s (got %s %s and %s %s)"
                              % (tuple(x.shape), tuple(m0.shape), m0.dtype, tuple(m1.shape), m1.dtype))
        src = _DT[m0.dtype]
    else:
        if m0.dtype != torch.float32 or m0.shape != x.shape:
            raise PwwHipError("sched_step: a single model output must be float32 of x's shape %s (got %s %s)" % (tuple(x.shape), tuple(m0.shape), m0.dtype))
        src = _lib.STEP_SRC_F32
    copies, out = 0, 0
    if u is not None:
        if u.dtype not in _DT or u.dim() != x.dim() or u.shape[1:] != x.shape[1:] or u.shape[0] % x.shape[0]:
            raise PwwHipError("sched_step: u must be float16 / bfloat16 [copies * n, ...] for x %s (got %s %s)" % (tuple(x.shape), tuple(u.shape), u.dtype))
        copies, out = u.shape[0] // x.shape[0], _DT[u.dtype]
    tensors = [t for t in (x, h, z, u, m0, m1) if t is not None]
    if not all(t.is_contiguous() for t in tensors):
        raise PwwHipError("sched_step needs contiguous tensors (x and h are written in place)")
    if len({t.device for t in tensors}) != 1:
        raise PwwHipError("sched_step needs its tensors on one device")
    lib = _lib.load_step()
    if lib is None:
        raise PwwHipError("libpww_hip_step.so not found at %s: ops.sched_step needs it %s" % (_lib.STEP_LIB_PATH, _lib._HINT))
    host = (ctypes.c_float * _lib.STEP_ROW)(*row)
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_step_fwd(_ptr(x), _ptr(h), _ptr(m0), _ptr(m1), float(guidance_scale), _ptr(z), _ptr(u), host, x.numel(), copies, src, out,
                                    _stream()), "pww_step_fwd", lib)
    STEP_LAUNCHES[0] += 1
    return x


# ---- GroupNorm (+ per-(image, channel) addend, + SiLU) of the blocks that call the attention path ------------------------------------
def group_norm(x, num_groups, weight=None, bias=None, eps=1e-5, add=None, act=None, workspace=None, out=None, pre_bias=None):
    """act(GroupNorm(x + add[:, :, None, None])) for a [B, C, H, W] float16 / bfloat16 tensor in NCHW-contiguous or channels_last memory
    format (the output has x's format); `add` [B, C] (unit stride along C; rows may be views into a wider tensor) or None; `pre_bias` [C] or
    None: a per-channel addend applied, and rounded, before `add` (the bias of the convolution that produced x); act None | "silu". SURVEY.md section 8 row a17 (diffusers 0.10.0 ResnetBlock2D / Transformer2DModel, the callers of the patched CrossAttention).
    The scratch for the partial sums (<= 1 MB; none for the single-launch form) comes from the caching allocator per call -- stream-ordered,
    so concurrent streams never share it and a hipGraph capture takes it from the graph's pool -- unless the caller passes `workspace`."""
    _require_gpu(x)
    if x.dim() != 4 or x.dtype not in _DT:
        raise PwwHipError("group_norm needs a 4-d float16/bfloat16 tensor (got %s %s)" % (tuple(x.shape), x.dtype))
    B, C, H, W = x.shape
    if x.is_contiguous():
        layout = _lib.LAYOUT_NCHW
    elif x.is_contiguous(memory_format=torch.channels_last):
        layout = _lib.LAYOUT_NHWC
    else:
        x = x.contiguous()
        layout = _lib.LAYOUT_NCHW
    if out is None:
        out = torch.empty_like(x)     # (preserves the memory format)
    elif out.shape != x.shape or out.dtype != x.dtype or out.stride() != x.stride():
        raise PwwHipError("group_norm: `out` must have x's shape, dtype and strides")
    for name, t, shape in (("weight", weight, (C,)), ("bias", bias, (C,)), ("add", add, (B, C)), ("pre_bias", pre_bias, (C,))):
        if t is not None and (t.dtype != x.dtype or tuple(t.shape) != shape or t.device != x.device):
            raise PwwHipError("group_norm: `%s` must be %s %s on %s (got %s %s)" % (name, x.dtype, shape, x.device, t.dtype, tuple(t.shape)))
    weight = weight.contiguous() if weight is not None else None
    bias = bias.contiguous() if bias is not None else None
    pre_bias = pre_bias.contiguous() if pre_bias is not None else None
    add_stride = 0
    if add is not None:
        if add.stride(1) != 1 or add.stride(0) % 8 != 0 or add.data_ptr() % 16 != 0:
            add = add.contiguous()
        add_stride = add.stride(0) if B > 1 else C
    if act not in (None, "silu"):
        raise PwwHipError("group_norm: act must be None or 'silu'")
    d = _lib.GnDesc(_DT[x.dtype], layout, B, C, H * W, int(num_groups), float(eps), _lib.ACT_SILU if act == "silu" else _lib.ACT_NONE, add_stride, 0)
    lib = _lib.load()
    need = lib.pww_group_norm_workspace_bytes(ctypes.byref(d))
    if need == 0:
        raise PwwHipError("group_norm: unsupported shape B %d C %d HW %d groups %d (C and H*W multiples of 8, C %% groups == 0, "
                          "groups <= 32, C <= 4096 in channels_last)" % (B, C, H * W, num_groups))
    ws = workspace if workspace is not None else torch.empty(int(need), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_group_norm_fwd(_ptr(x), _ptr(pre_bias), _ptr(add), _ptr(weight), _ptr(bias), _ptr(out), ctypes.byref(d), _ptr(ws), ws.numel(),
                                          _stream()), "pww_group_norm_fwd")
    return out


def _rows(t, name):
    """[..., C] tensor as rows: (rows, C, row stride) -- unit stride along C, ONE stride between consecutive rows."""
    if t.dtype not in _DT or t.dim() < 2:
        raise PwwHipError("%s: a float16/bfloat16 tensor of at least two dims is needed (got %s %s)" % (name, t.dtype, tuple(t.shape)))
    if t.stride(-1) != 1 or t.stride(-2) % 8 != 0 or t.data_ptr() % 16 != 0:
        return None                                 # (the caller makes it contiguous: e.g. the [B, HW, C] view of an NCHW tensor)
    C = t.shape[-1]
    rows = t.numel() // C
    stride = t.stride(-2)
    exp = stride
    for d in range(t.dim() - 2, -1, -1):          # every leading dim must continue the same row pitch
        if t.shape[d] != 1 and t.stride(d) != exp:
            return None
        exp *= t.shape[d]
    return rows, C, stride


def add_layer_norm(x, weight, bias, eps, a=None, post_bias=None):
    """LayerNorm over the last dim of x ([..., C]); with `a` (same shape): s = a + x, returns (s, LayerNorm(s)) from ONE launch -- the
    `attn(norm(h)) + h` of diffusers' BasicTransformerBlock together with the block's next norm. Without `a`: returns LayerNorm(x).
    post_bias ([C], with `a`): the returned sum is s + post_bias (the LayerNorm still is that of s): the bias of the GEMM whose output the
    caller adds to it next, through that GEMM's C operand."""
    _require_gpu(x)
    rx = _rows(x, "add_layer_norm")
    if rx is None:
        x = x.contiguous()
        rx = _rows(x, "add_layer_norm")
    if rx is None:                                  # (contiguous rows that still do not qualify: C no multiple of 8)
        raise PwwHipError("add_layer_norm: the last dim must be a multiple of 8 (got %d)" % x.shape[-1])
    rows, C, xs = rx
    ra = None
    if a is not None:
        if a.shape != x.shape or a.dtype != x.dtype:
            raise PwwHipError("add_layer_norm: `a` must have x's shape and dtype")
        ra = _rows(a, "add_layer_norm")
        if ra is None:
            a = a.contiguous()
            ra = _rows(a, "add_layer_norm")
    for name, t in (("weight", weight), ("bias", bias), ("post_bias", post_bias)):
        if t is not None and (t.dtype != x.dtype or tuple(t.shape) != (C,) or not t.is_contiguous()):
            raise PwwHipError("add_layer_norm: `%s` must be a contiguous %s [%d]" % (name, x.dtype, C))
    if post_bias is not None and a is None:
        raise PwwHipError("add_layer_norm: post_bias needs the add form (a)")
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    s = torch.empty(x.shape, dtype=x.dtype, device=x.device) if a is not None else None
    d = _lib.LnDesc(_DT[x.dtype], C, rows, ra[2] if ra else 0, xs, C, C, float(eps), 0)
    with torch.cuda.device(x.device):
        if post_bias is not None:
            _lib.check(_lib.load().pww_add_layer_norm_bias(_ptr(a), _ptr(x), _ptr(weight), _ptr(bias), _ptr(post_bias), _ptr(s), _ptr(y), ctypes.byref(d),
                                                           _stream()), "pww_add_layer_norm_bias")
        else:
            _lib.check(_lib.load().pww_add_layer_norm(_ptr(a), _ptr(x), _ptr(weight), _ptr(bias), _ptr(s), _ptr(y), ctypes.byref(d), _stream()),
                       "pww_add_layer_norm")
    return (s, y) if a is not None else y


def geglu(h):
    """h[..., :D] * gelu(h[..., D:]) for the output of GEGLU's projection (diffusers FeedForward.net[0]); erf form of gelu."""
    _require_gpu(h)
    r = _rows(h, "geglu")
    if r is None:
        h = h.contiguous()
        r = _rows(h, "geglu")
    if r is None:
        raise PwwHipError("geglu: the last dim must be 2 * D with D a multiple of 8 (got %d)" % h.shape[-1])
    rows, C2, hs = r
    if C2 % 16 != 0:
        raise PwwHipError("geglu: the last dim must be 2 * D with D a multiple of 8 (got %d)" % C2)
    D = C2 // 2
    y = torch.empty(h.shape[:-1] + (D,), dtype=h.dtype, device=h.device)
    with torch.cuda.device(h.device):
        _lib.check(_lib.load().pww_geglu(_ptr(h), _ptr(y), rows, D, hs, D, _DT[h.dtype], _stream()), "pww_geglu")
    return y


def bias_residual(residual, value, bias):
    """residual + (value + bias[None, :, None, None]) for [B, C, H, W] tensors of ONE memory format (NCHW-contiguous or channels_last), the two
    roundings of the stock sequence kept; one launch."""
    _require_gpu(residual, value, bias)
    if residual.shape != value.shape or residual.dtype != value.dtype or residual.dtype not in _DT or residual.dim() != 4 or bias.dtype != residual.dtype:
        raise PwwHipError("bias_residual: two same-shape 4-d float16/bfloat16 tensors and a bias of that type are needed")
    B, C, H, W = residual.shape
    if tuple(bias.shape) != (C,):
        raise PwwHipError("bias_residual: bias must have shape (%d,), got %s" % (C, tuple(bias.shape)))
    nhwc = value.is_contiguous(memory_format=torch.channels_last) and not value.is_contiguous()
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    value, residual = value.contiguous(memory_format=fmt), residual.contiguous(memory_format=fmt)       # (no-ops when both already are)
    layout = _lib.LAYOUT_NHWC if nhwc else _lib.LAYOUT_NCHW
    y = torch.empty_like(value)
    with torch.cuda.device(value.device):
        _lib.check(_lib.load().pww_bias_residual(_ptr(residual), _ptr(value), _ptr(bias.contiguous()), _ptr(y), B, C, H * W, layout, _DT[value.dtype], _stream()),
                   "pww_bias_residual")
    return y


def _khwc_weight(weight):
    """The [Cout][3][3][Cin] storage the conv kernel reads: a channels_last weight IS that storage; any other layout gets a repacked copy, cached
    on the parameter and rebuilt when it was replaced, modified in place (version counter), moved or cast."""
    if weight.is_contiguous(memory_format=torch.channels_last):
        return weight
    key = (weight.data_ptr(), weight._version, weight.dtype, weight.device)
    hit = weight.__dict__.get("_pww_khwc")
    if hit is not None and hit[0] == key:
        return hit[1]
    packed = weight.detach().permute(0, 2, 3, 1).contiguous()
    weight.__dict__["_pww_khwc"] = (key, packed)
    return packed


def conv3x3_takes(x, weight, stride=1, upsample=False):
    """True when pww_conv3x3_fwd runs this call: a channels_last 4-d float16 / bfloat16 x on a HIP device, a [Cout, Cin, 3, 3] weight of its dtype,
    Cin a multiple of 64, Cout a multiple of 64 or of 160 (the kernel's tile widths: 64, 128, 160), stride 1 or 2 (upsample: stride 1)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in _DT and torch.is_tensor(weight) and weight.dtype == x.dtype and weight.dim() == 4):
        return False
    B, C, H, W = x.shape
    Cout = weight.shape[0]
    return (tuple(weight.shape[1:]) == (C, 3, 3) and C % 64 == 0 and (Cout % 64 == 0 or Cout % 160 == 0) and Cout >= 64 and stride in (1, 2) and not (upsample and stride != 1)
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0
            and B * H * W * C < 2 ** 31 // 4)


def conv3x3(x, weight, bias=None, residual=None, stride=1, upsample=False, tile_n=0, splitk=0):
    """3 x 3 convolution, padding 1, of a channels_last x ([B, Cin, H, W]) -> channels_last [B, Cout, Ho, Wo] on one HIP implicit-GEMM kernel
    (+ a fold launch when the K dimension is split). upsample: the input is first upsampled 2x nearest (fused into the gather). Epilogue with
    the stock roundings: T(residual + T(T(conv) + bias)), each term when given. tile_n / splitk: 0 = the library's choice (A/B and tools)."""
    _require_gpu(x, weight, bias, residual)
    if not conv3x3_takes(x, weight, stride, upsample):
        raise PwwHipError("conv3x3: needs a channels_last float16/bfloat16 x with Cin, Cout multiples of 64 and a 3 x 3 weight of its dtype")
    B, C, H, W = x.shape
    Cout = weight.shape[0]
    Hv, Wv = H << int(bool(upsample)), W << int(bool(upsample))
    Ho, Wo = (Hv - 1) // stride + 1, (Wv - 1) // stride + 1
    w = _khwc_weight(weight)
    if bias is not None and (bias.dtype != x.dtype or tuple(bias.shape) != (Cout,)):
        raise PwwHipError("conv3x3: bias must be a %s [%d]" % (x.dtype, Cout))
    if bias is not None:
        bias = bias.contiguous()
    if residual is not None:
        if tuple(residual.shape) != (B, Cout, Ho, Wo) or residual.dtype != x.dtype:
            raise PwwHipError("conv3x3: residual must be a %s %s" % (x.dtype, (B, Cout, Ho, Wo)))
        residual = residual.contiguous(memory_format=torch.channels_last)
    d = _lib.ConvDesc(ctypes.sizeof(_lib.ConvDesc), _DT[x.dtype], B, H, W, C, Cout, int(stride), int(bool(upsample)), int(tile_n), int(splitk), 0)
    lib = _lib.load()
    # the same entry points under another name where the plan is the 160-wide tile: its code objects live in libpww_hip_convwide.so
    # (a required library: loading it raises when it is missing)
    side = _lib.load_convwide()
    wide = side.pww_convwide_takes(ctypes.byref(d)) == 1
    ws_bytes, fwd, what = ((side.pww_convwide_workspace_bytes, side.pww_convwide_fwd, "pww_convwide_fwd") if wide else
                           (lib.pww_conv3x3_workspace_bytes, lib.pww_conv3x3_fwd, "pww_conv3x3_fwd"))
    y = torch.empty((B, Cout, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    nbytes = int(ws_bytes(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    with torch.cuda.device(x.device):
        rc = fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(y), ctypes.byref(d), _ptr(ws), nbytes, _stream())
        if wide:
            _lib.check(rc, what, side)
        else:
            _lib.check(rc, what)
    return y


# ---- conv2 of a ResnetBlock2D with the block's 1 x 1 shortcut as further K-slabs (csrc/pww_conv_tail.hip, libpww_hip_convtail.so) -------
def conv3x3_shortcut_takes(h, conv2_weight, x, shortcut_weight):
    """True when pww_convtail_fwd runs this call: what conv3x3_takes asks of (h, conv2_weight) at stride 1, and a channels_last x of h's
    dtype, device, batch and size whose channel count C2 is a multiple of 64, with a dense [Cout, C2, 1, 1] (or [Cout, C2]) weight of that dtype."""
    if not (conv3x3_takes(h, conv2_weight) and torch.is_tensor(x) and x.is_cuda and x.device == h.device and x.dim() == 4 and x.dtype == h.dtype
            and torch.is_tensor(shortcut_weight) and shortcut_weight.dtype == h.dtype and shortcut_weight.device == h.device):
        return False
    w2 = _linear_weight(shortcut_weight)
    B, C2, H, W = x.shape
    return (w2 is not None and tuple(w2.shape) == (conv2_weight.shape[0], C2) and C2 % 64 == 0 and (B, H, W) == (h.shape[0], h.shape[2], h.shape[3])
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0 and B * H * W * C2 < 2 ** 31 // 4)


def conv3x3_shortcut(h, conv2_weight, conv2_bias, x, shortcut_weight, shortcut_bias, tile_n=0, splitk=0):
    """conv3x3(h, conv2_weight) + conv1x1(x, shortcut_weight) + conv2_bias + shortcut_bias for channels_last h ([B, Cin, H, W]) and x
    ([B, C2, H, W]) -> channels_last [B, Cout, H, W]: ONE implicit GEMM over 9 Cin + C2 (+ a fold launch when K is split), the shortcut's
    output never a tensor. fp32 accumulation, one rounding: T(acc + conv2_bias + shortcut_bias). tile_n / splitk: 0 = the library's choice."""
    _require_gpu(h, conv2_weight, conv2_bias, x, shortcut_weight, shortcut_bias)
    if not conv3x3_shortcut_takes(h, conv2_weight, x, shortcut_weight):
        raise PwwHipError("conv3x3_shortcut: needs channels_last float16/bfloat16 h and x of one dtype, batch and size, channel counts multiples of 64, "
                          "a 3 x 3 weight and a dense 1 x 1 weight of that dtype")
    B, C, H, W = h.shape
    Cout, C2 = conv2_weight.shape[0], x.shape[1]
    w = _khwc_weight(conv2_weight)
    w2 = _linear_weight(shortcut_weight)
    biases = []
    for name, b in (("conv2_bias", conv2_bias), ("shortcut_bias", shortcut_bias)):
        if not torch.is_tensor(b) or b.dtype != h.dtype or tuple(b.shape) != (Cout,):
            raise PwwHipError("conv3x3_shortcut: %s must be a %s [%d]" % (name, h.dtype, Cout))
        biases.append(b.contiguous() if b.data_ptr() % 8 == 0 else b.clone(memory_format=torch.contiguous_format))
    lib = _lib.load_convtail()
    if lib is None:
        raise PwwHipError("conv3x3_shortcut: libpww_hip_convtail.so is not built %s" % _lib._HINT)
    d = _lib.ConvTailDesc(ctypes.sizeof(_lib.ConvTailDesc), _DT[h.dtype], B, H, W, C, C2, Cout, int(tile_n), int(splitk))
    y = torch.empty((B, Cout, H, W), dtype=h.dtype, device=h.device, memory_format=torch.channels_last)
    nbytes = int(lib.pww_convtail_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=h.device) if nbytes else None
    with torch.cuda.device(h.device):
        _lib.check(lib.pww_convtail_fwd(_ptr(h), _ptr(w), _ptr(x), _ptr(w2), _ptr(biases[0]), _ptr(biases[1]), _ptr(y), ctypes.byref(d), _ptr(ws), nbytes,
                                        _stream()), "pww_convtail_fwd", lib)
    return y


# ---- the two readers of torch.cat([x1, x2], 1) in an up block, reading the halves where they lie (csrc/pww_concat.hip, libpww_hip_concat.so)
def _cat_pair(x1, x2, grid):
    """Two channels_last 4-d float16 / bfloat16 tensors of one dtype, device, batch and size on a HIP device, 16-byte aligned, their channel
    counts multiples of `grid`: what both two-source kernels ask of the pair."""
    if not (torch.is_tensor(x1) and torch.is_tensor(x2) and x1.is_cuda and x1.device == x2.device and x1.dim() == 4 and x2.dim() == 4
            and x1.dtype in _DT and x2.dtype == x1.dtype):
        return False
    (B, C1, H, W), C2 = x1.shape, x2.shape[1]
    return ((x2.shape[0], x2.shape[2], x2.shape[3]) == (B, H, W) and C1 % grid == 0 and C2 % grid == 0 and C1 > 0 and C2 > 0
            and x1.is_contiguous(memory_format=torch.channels_last) and x2.is_contiguous(memory_format=torch.channels_last)
            and x1.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0)


def _gn_cat_desc(x1, x2, num_groups, eps, act):
    B, C1, H, W = x1.shape
    return _lib.ConcatGnDesc(ctypes.sizeof(_lib.ConcatGnDesc), _DT[x1.dtype], B, C1, x2.shape[1], H * W, int(num_groups), float(eps),
                             _lib.ACT_SILU if act == "silu" else _lib.ACT_NONE, 0)


def group_norm_cat_takes(x1, x2, num_groups, weight=None, bias=None):
    """True when pww_concat_group_norm_fwd runs this call: a pair as `_cat_pair` describes it with channel counts on the 8 grid, affine
    parameters of its dtype (or none), a shape group_norm takes for C1 + C2 channels in channels_last, and the side library there."""
    if not _cat_pair(x1, x2, 8):
        return False
    C = x1.shape[1] + x2.shape[1]
    for t in (weight, bias):
        if t is not None and not (torch.is_tensor(t) and t.dtype == x1.dtype and tuple(t.shape) == (C,) and t.device == x1.device):
            return False
    lib = _lib.load_concat()
    return lib is not None and int(lib.pww_concat_group_norm_workspace_bytes(ctypes.byref(_gn_cat_desc(x1, x2, num_groups, 1e-5, None)))) > 0


def group_norm_cat(x1, x2, num_groups, weight=None, bias=None, eps=1e-5, act=None, workspace=None):
    """group_norm(torch.cat([x1, x2], 1), ...) for two channels_last tensors without the concatenation: the same launch form, summation
    order and roundings, so the same bits. The output is a channels_last [B, C1 + C2, H, W]. act None | "silu"."""
    _require_gpu(x1, x2)
    if act not in (None, "silu"):
        raise PwwHipError("group_norm_cat: act must be None or 'silu'")
    if not group_norm_cat_takes(x1, x2, num_groups, weight, bias):
        raise PwwHipError("group_norm_cat: needs two channels_last float16/bfloat16 tensors of one dtype, batch and size with channel counts multiples "
                          "of 8, C1 + C2 a shape group_norm takes, and libpww_hip_concat.so %s" % _lib._HINT)
    B, C1, H, W = x1.shape
    weight = weight.contiguous() if weight is not None else None
    bias = bias.contiguous() if bias is not None else None
    d = _gn_cat_desc(x1, x2, num_groups, eps, act)
    lib = _lib.load_concat()
    need = int(lib.pww_concat_group_norm_workspace_bytes(ctypes.byref(d)))
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=x1.device)
    out = torch.empty((B, C1 + x2.shape[1], H, W), dtype=x1.dtype, device=x1.device, memory_format=torch.channels_last)
    with torch.cuda.device(x1.device):
        _lib.check(lib.pww_concat_group_norm_fwd(_ptr(x1), _ptr(x2), _ptr(weight), _ptr(bias), _ptr(out), ctypes.byref(d), _ptr(ws), ws.numel(), _stream()),
                   "pww_concat_group_norm_fwd", lib)
    return out


def conv3x3_shortcut_cat_takes(h, conv2_weight, x1, x2, shortcut_weight):
    """True when pww_concat_convtail_fwd runs this call: what conv3x3_shortcut_takes asks of (h, conv2_weight, torch.cat([x1, x2], 1),
    shortcut_weight), with both parts on the 64-channel grid, and the side library there."""
    if not (conv3x3_takes(h, conv2_weight) and _cat_pair(x1, x2, 64) and x1.device == h.device and x1.dtype == h.dtype
            and torch.is_tensor(shortcut_weight) and shortcut_weight.dtype == h.dtype and shortcut_weight.device == h.device):
        return False
    w2 = _linear_weight(shortcut_weight)
    B, C1, H, W = x1.shape
    Ct = C1 + x2.shape[1]
    return (w2 is not None and tuple(w2.shape) == (conv2_weight.shape[0], Ct) and (B, H, W) == (h.shape[0], h.shape[2], h.shape[3])
            and B * H * W * Ct < 2 ** 31 // 4 and _lib.load_concat() is not None)


def conv3x3_shortcut_cat(h, conv2_weight, conv2_bias, x1, x2, shortcut_weight, shortcut_bias, tile_n=0, splitk=0):
    """conv3x3_shortcut(h, conv2_weight, conv2_bias, torch.cat([x1, x2], 1), shortcut_weight, shortcut_bias) without the concatenation: the
    same tile, K order, split and epilogue, so the same bits. tile_n / splitk: 0 = the choice conv3x3_shortcut makes."""
    _require_gpu(h, conv2_weight, conv2_bias, x1, x2, shortcut_weight, shortcut_bias)
    if not conv3x3_shortcut_cat_takes(h, conv2_weight, x1, x2, shortcut_weight):
        raise PwwHipError("conv3x3_shortcut_cat: needs channels_last float16/bfloat16 h, x1 and x2 of one dtype, batch and size, channel counts multiples "
                          "of 64, a 3 x 3 weight and a dense 1 x 1 weight of that dtype over C1 + C2 channels, and libpww_hip_concat.so %s" % _lib._HINT)
    B, C, H, W = h.shape
    Cout = conv2_weight.shape[0]
    w = _khwc_weight(conv2_weight)
    w2 = _linear_weight(shortcut_weight)
    biases = []
    for name, b in (("conv2_bias", conv2_bias), ("shortcut_bias", shortcut_bias)):
        if not torch.is_tensor(b) or b.dtype != h.dtype or tuple(b.shape) != (Cout,):
            raise PwwHipError("conv3x3_shortcut_cat: %s must be a %s [%d]" % (name, h.dtype, Cout))
        biases.append(b.contiguous() if b.data_ptr() % 8 == 0 else b.clone(memory_format=torch.contiguous_format))
    lib = _lib.load_concat()
    d = _lib.ConcatTailDesc(ctypes.sizeof(_lib.ConcatTailDesc), _DT[h.dtype], B, H, W, C, x1.shape[1], x2.shape[1], Cout, int(tile_n), int(splitk), 0)
    y = torch.empty((B, Cout, H, W), dtype=h.dtype, device=h.device, memory_format=torch.channels_last)
    nbytes = int(lib.pww_concat_convtail_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=h.device) if nbytes else None
    with torch.cuda.device(h.device):
        _lib.check(lib.pww_concat_convtail_fwd(_ptr(h), _ptr(w), _ptr(x1), _ptr(x2), _ptr(w2), _ptr(biases[0]), _ptr(biases[1]), _ptr(y), ctypes.byref(d),
                                               _ptr(ws), nbytes, _stream()), "pww_concat_convtail_fwd", lib)
    return y


# ---- linear layers with the post-processing of the GEMM's output in its epilogue (csrc/pww_linear.hip, libpww_hip_linear.so) ------------
def _linear_weight(weight):
    """[N, K] view of an nn.Linear weight or of a 1 x 1 conv weight ([N, K, 1, 1]), in place; None when it is neither or not dense."""
    if not torch.is_tensor(weight) or weight.dim() not in (2, 4) or (weight.dim() == 4 and tuple(weight.shape[2:]) != (1, 1)):
        return None
    w = weight.detach().reshape(weight.shape[0], weight.shape[1]) if weight.dim() == 4 else weight.detach()
    return w if w.is_contiguous() and w.data_ptr() == weight.data_ptr() and w.data_ptr() % 16 == 0 else None


def linear_takes(x, weight, geglu=False, bias=None, residual=None, out=None):
    """True when pww_linear_fwd runs this call -- everything the library would answer PWW_ENOTSUP or PWW_EINVAL to is declined here: a
    float16 / bfloat16 [..., K] x on a HIP device whose rows have one pitch (unit stride along K, a multiple of 8 elements, 16-byte aligned),
    a dense [N, K] (or [N, K, 1, 1]) weight of its dtype, K and N multiples of 64 (geglu: N / 2 a multiple of 64); where given, a dense
    8-byte aligned bias [N] of that dtype, and a residual / `out` of the output's shape and dtype whose rows have one such pitch too."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in _DT and x.dim() >= 2 and torch.is_tensor(weight) and weight.dtype == x.dtype):
        return False
    w = _linear_weight(weight)
    if w is None or x.shape[-1] != w.shape[1] or x.numel() == 0 or _rows(x, "linear") is None:
        return False
    N, K = w.shape
    rows, _, xs = _rows(x, "linear")
    if not (K % 64 == 0 and N % (128 if geglu else 64) == 0 and rows * xs < 2 ** 31 and rows * N < 2 ** 31 and N * K < 2 ** 31):
        return False
    if bias is not None and not (torch.is_tensor(bias) and bias.is_cuda and bias.dtype == x.dtype and tuple(bias.shape) == (N,) and bias.is_contiguous()
                                 and bias.data_ptr() % 8 == 0):
        return False
    shape = tuple(x.shape[:-1]) + (N // 2 if geglu else N,)
    for t in (residual, out):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == x.dtype and tuple(t.shape) == shape and _rows(t, "linear") is not None):
            return False
    return True


def linear(x, weight, bias=None, residual=None, geglu=False, tile_n=0, splitk=0, out=None):
    """F.linear(x, weight, bias) (+ residual), or with geglu=True GEGLU of it (`v * gelu(gate)`, [v | gate] = the two halves of the output
    channels), on one HIP GEMM kernel (+ a fold launch when the K dimension is split). Rounding points: T(T(acc) + bias) (the accumulator is
    rounded before the bias is added), then those of the unfused sequence on it: T(residual + that), T(v * T(gelu(gate))). weight: [N, K] or
    a 1 x 1 conv weight [N, K, 1, 1], read in place. x, residual and `out` (default: a new dense tensor) are [..., C] tensors whose rows have
    one pitch. tile_n / splitk: 0 = the library's choice."""
    _require_gpu(x, weight, bias, residual, out)
    if not linear_takes(x, weight, geglu):
        raise PwwHipError("linear: needs a float16/bfloat16 [..., K] x with one row pitch and a dense [N, K] weight of its dtype, K and N multiples of 64%s"
                          % (" (geglu: N / 2 a multiple of 64)" if geglu else ""))
    w = _linear_weight(weight)
    N, K = w.shape
    M, _, xs = _rows(x, "linear")
    nout = N // 2 if geglu else N
    if (geglu or residual is not None) and bias is None:
        raise PwwHipError("linear: the residual and GEGLU epilogues need the bias")
    if geglu and residual is not None:
        raise PwwHipError("linear: geglu and residual exclude each other")
    if bias is not None:
        if bias.dtype != x.dtype or tuple(bias.shape) != (N,):
            raise PwwHipError("linear: bias must be a %s [%d]" % (x.dtype, N))
        bias = bias.contiguous() if bias.data_ptr() % 8 == 0 else bias.clone(memory_format=torch.contiguous_format)
    shape = tuple(x.shape[:-1]) + (nout,)
    rs = 0
    if residual is not None:
        if tuple(residual.shape) != shape or residual.dtype != x.dtype:
            raise PwwHipError("linear: residual must be a %s %s" % (x.dtype, shape))
        r = _rows(residual, "linear")
        if r is None:
            residual = residual.contiguous()
            r = _rows(residual, "linear")
        rs = r[2]
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != x.dtype or _rows(out, "linear") is None:
        raise PwwHipError("linear: out must be a %s %s whose rows have one pitch" % (x.dtype, shape))
    ys = _rows(out, "linear")[2]
    epi = _lib.LINEAR_BIAS_GEGLU if geglu else _lib.LINEAR_BIAS_RESIDUAL if residual is not None else _lib.LINEAR_BIAS if bias is not None else _lib.LINEAR_NONE
    d = _lib.LinearDesc(ctypes.sizeof(_lib.LinearDesc), _DT[x.dtype], M, N, K, epi, xs, ys, rs, int(tile_n), int(splitk))
    lib = _lib.load_linear()
    nbytes = int(lib.pww_linear_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_linear_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out), ctypes.byref(d), _ptr(ws), nbytes, _stream()), "pww_linear_fwd", lib)
    return out


# ---- the per-row low-rank update of unmerged LoRA adapters (csrc/pww_lora.hip, libpww_hip_lora.so) -------------------------------------
def lora_update_torch(y, x, A, B, row_adapter, row_scale, n_seg):
    """pww_lora_fwd's formula from stock torch ops, in place on y (any device, any float dtype): per adapter and segment two matmuls (the
    first one's output is a tensor of y's dtype, i.e. rounded once) and the scaled add in at least fp32, rounded once. The rows are selected
    by a mask instead of gathered -- no shape depends on the assignment, so this too is legal under stream capture -- and a row without an
    adapter (or with scale 0) keeps its bits."""
    R, ns = y.shape[0], y.shape[-1] // n_seg
    ra, rs = row_adapter[:R].reshape(R, 1, 1), row_scale[:R].reshape(R, 1, 1)
    wide = torch.promote_types(y.dtype, torch.float32)
    for i in range(A.shape[0]):
        on = (ra == i) & (rs != 0)
        for g in range(n_seg):
            u = torch.matmul(torch.matmul(x, A[i, g].t()), B[i, g].t())
            seg = y[..., g * ns:(g + 1) * ns]
            seg.copy_(torch.where(on, (seg.to(wide) + rs.to(wide) * u.to(wide)).to(y.dtype), seg))
    return y


def lora_takes(y, x, A, B, n_seg):
    """True when pww_lora_fwd runs this update -- everything the library would answer PWW_ENOTSUP or PWW_EINVAL to is declined here."""
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype in _DT and y.dim() == 3 and x.dim() == 3 and x.dtype == y.dtype == A.dtype == B.dtype
            and x.is_cuda and A.is_cuda and B.is_cuda and A.is_contiguous() and B.is_contiguous() and A.dim() == 4 and B.dim() == 4):
        return False
    (R, T, N), K, (n, seg, rank, _) = y.shape, x.shape[-1], A.shape
    if not (tuple(x.shape[:2]) == (R, T) and seg == n_seg and 1 <= n_seg <= _lib.LORA_MAX_SEGMENTS and 1 <= n <= _lib.LORA_MAX_ADAPTERS and A.shape[3] == K
            and N % n_seg == 0 and tuple(B.shape) == (n, n_seg, N // n_seg, rank) and rank in (32, 64, 96, 128) and K % 32 == 0 and (N // n_seg) % 16 == 0
            and 1 <= R <= 65535 and T >= 1):
        return False
    for t, w in ((x, K), (y, N)):
        rs, ts = (T * t.stride(1) if R == 1 else t.stride(0)), t.stride(1)
        if t.stride(2) != 1 or ts < w or rs < T * ts or rs % 8 or ts % 8 or t.data_ptr() % 16 or R * rs >= 2 ** 31:
            return False
    return A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0 and A.numel() < 2 ** 31 and B.numel() < 2 ** 31


def lora_update(y, x, layer_stack, state, n_seg):
    """y += s (x A^T) B^T per row, in place: y [R, T, N] (a view of a wider buffer is fine), x [R, T, K], layer_stack = (A [n][n_seg][rank][K],
    B [n][n_seg][N / n_seg][rank]) (lora.LoraLayer.stack), the row's adapter and scale from `state` (lora.LoraState: row_adapter / row_scale,
    device arrays the launch reads when it RUNS). One launch of libpww_hip_lora.so where it takes the operands; anything else runs
    lora_update_torch and is counted as declined (lora.stats())."""
    from . import lora as _lora
    A, B = layer_stack
    if x.dtype != y.dtype:
        x = x.to(y.dtype)
    if A.dtype != y.dtype:      # (autocast: the projections ran in another dtype than the UNet's)
        A, B = A.to(y.dtype), B.to(y.dtype)
    if x.dim() == 3 and (x.stride(2) != 1 or x.stride(1) % 8 or (x.shape[0] > 1 and (x.stride(0) % 8 or x.stride(0) < x.shape[1] * x.stride(1))) or x.data_ptr() % 16):
        x = x.contiguous()
    state._ensure_rows()
    if y.shape[0] > state.row_adapter.numel():
        raise PwwHipError("lora_update: %d rows, the assignment holds %d" % (y.shape[0], state.row_adapter.numel()))
    if not lora_takes(y, x, A, B, n_seg):
        _lora._stats["declined"] += 1
        return lora_update_torch(y, x, A, B, state.row_adapter, state.row_scale, n_seg)
    (R, T, N), K = y.shape, x.shape[-1]
    d = _lib.LoraDesc(ctypes.sizeof(_lib.LoraDesc), _DT[y.dtype], R, T, K, N, n_seg, A.shape[2], A.shape[0], 0,
                      T * x.stride(1) if R == 1 else x.stride(0), x.stride(1), T * y.stride(1) if R == 1 else y.stride(0), y.stride(1))
    lib = _lib.load_lora()
    with torch.cuda.device(y.device):
        _lib.check(lib.pww_lora_fwd(_ptr(x), _ptr(A), _ptr(B), _ptr(state.row_adapter), _ptr(state.row_scale), _ptr(y), ctypes.byref(d), _stream()),
                   "pww_lora_fwd", lib)
    _lora._stats["kernel"] += 1
    return y


# ---- the residuals of a ControlNet as one grouped GEMM (csrc/pww_control.hip, libpww_hip_control.so) -------------------------------------
CONTROL_MAX_PROBLEMS = _lib.CONTROL_MAX_PROBLEMS
CONTROL_LAUNCHES = [0, 0]           # grouped launches, problems they held (pww_hip.controlnet.stats() reports them)


def _nhwc_rows(t):
    """A [B, C, H, W] float16 / bfloat16 tensor as the [B H W, C] rows of its channels_last memory: (rows, C, row pitch), or None when the
    channels are not adjacent, the pixels do not follow each other at ONE pitch (a slice of the channels of a wider channels_last tensor
    does), the pitch is no multiple of 8 elements or the first element is not 16-byte aligned. Nothing is copied."""
    if not torch.is_tensor(t) or t.dim() != 4 or t.dtype not in _DT or t.data_ptr() % 16 or t.numel() == 0:
        return None
    B, C, H, W = t.shape
    if C > 1 and t.stride(1) != 1:
        return None
    pitch = exp = None
    for size, stride in ((W, t.stride(3)), (H, t.stride(2)), (B, t.stride(0))):
        if size == 1:
            continue
        if pitch is None:
            pitch, exp = stride, stride * size
        elif stride != exp:
            return None
        else:
            exp *= size
    pitch = C if pitch is None else pitch
    return None if pitch % 8 or pitch < C else (B * H * W, C, pitch)


def _control_why_not(hs, convs, scale_word, skips=None, outs=None):
    """None when pww_control_fwd runs this call, else the reason it would not (one line, for controlnet.stats())."""
    n = len(hs)
    if not 1 <= n <= CONTROL_MAX_PROBLEMS or len(convs) != n:
        return "%d hidden states for %d zero convolutions (1 .. %d of each)" % (n, len(convs), CONTROL_MAX_PROBLEMS)
    if not (torch.is_tensor(scale_word) and scale_word.is_cuda and scale_word.dtype == torch.float32 and scale_word.numel() >= 1 and scale_word.data_ptr() % 4 == 0):
        return "the scale word must be a float32 tensor on the device"
    dt = hs[0].dtype if torch.is_tensor(hs[0]) else None
    for name, seq in (("skips", skips), ("outs", outs)):
        if seq is not None and len(seq) != n:
            return "%d %s for %d hidden states" % (len(seq), name, n)
    for p, (h, conv) in enumerate(zip(hs, convs)):
        w, b = getattr(conv, "weight", None), getattr(conv, "bias", None)
        if not (torch.is_tensor(h) and h.is_cuda and h.dtype in _DT and h.dtype == dt and h.device == scale_word.device):
            return "hidden state %d is not a float16 / bfloat16 tensor of one dtype on the scale word's device" % p
        rows = _nhwc_rows(h)
        if rows is None:
            return "hidden state %d is not a channels_last [B, C, H, W] tensor with one row pitch (a multiple of 8), 16-byte aligned" % p
        M, K, _ = rows
        wv = _linear_weight(w) if torch.is_tensor(w) and w.is_cuda and w.dtype == dt and w.dim() == 4 else None
        if wv is None or wv.shape[1] != K:
            return "zero convolution %d is not a dense 1 x 1 weight of the hidden state's dtype and channels" % p
        N = wv.shape[0]
        if K % 64 or N % 64:
            return "problem %d: K = %d and N = %d must be multiples of 64" % (p, K, N)
        if not (torch.is_tensor(b) and b.is_cuda and b.dtype == dt and tuple(b.shape) == (N,) and b.is_contiguous() and b.data_ptr() % 8 == 0):
            return "zero convolution %d has no dense, 8-byte aligned bias of its dtype" % p
        if M * rows[2] >= 2 ** 31 or N * K >= 2 ** 31:
            return "problem %d: tensor of 2^31 elements or more" % p
        for name, seq in (("skip", skips), ("out", outs)):
            t = None if seq is None else seq[p]
            if t is None:
                continue
            r = _nhwc_rows(t) if torch.is_tensor(t) and t.is_cuda and t.dtype == dt else None
            if r is None or tuple(t.shape) != (h.shape[0], N) + tuple(h.shape[2:]) or M * r[2] >= 2 ** 31:
                return "%s %d is not a channels_last [B, %d, H, W] tensor of the hidden state's dtype and size with one row pitch" % (name, p, N)
    return None


def control_takes(hs, convs, scale_word, skips=None, outs=None):
    """True when ops.control_residuals runs this call on the grouped kernel -- everything the library would answer PWW_ENOTSUP or PWW_EINVAL
    to is declined here, and so is a missing libpww_hip_control.so: 1 .. 16 channels_last [B, C, H, W] float16 / bfloat16 hidden states on a
    HIP device, taken as their [B H W, C] rows (one pitch, a multiple of 8 elements, 16-byte aligned), as many plain 1 x 1 nn.Conv2d (dense
    weight and bias of that dtype, channel counts multiples of 64), a float32 scale word on the device; where given, skips / outs of the
    outputs' shape with one row pitch too (an entry may be None)."""
    return _control_why_not(hs, convs, scale_word, skips, outs) is None and _lib.load_control() is not None


def control_residuals(hs, convs, scale_word, skips=None, outs=None):
    """out_p = T(skip_p + s * conv_p(h_p)) for every p (skips None, or an entry None: T(s * conv_p(h_p))), s = scale_word[0] as the device
    holds it when the launch RUNS -- a captured graph follows the word. ONE launch for all problems, fp32 accumulation, one rounding at the
    store; s == 0 returns the skips bit for bit. hs / skips / outs: [B, C, H, W] channels_last tensors read and written in place as their
    [B H W, C] rows (nothing is copied); convs: the 1 x 1 nn.Conv2d modules, weights used in place. outs default to new channels_last tensors
    (an out may be its skip). Returns the list of outs. Raises where control_takes declines."""
    _require_gpu(*[t for t in hs if torch.is_tensor(t)])
    why = _control_why_not(hs, convs, scale_word, skips, outs)
    if why is not None:
        raise PwwHipError("control_residuals: " + why)
    lib = _lib.load_control()
    if lib is None:
        raise PwwHipError("control_residuals: libpww_hip_control.so is not built " + _lib._HINT)
    n = len(hs)
    table = (_lib.ControlProblem * n)()
    result = []
    for p, (h, conv) in enumerate(zip(hs, convs)):
        M, K, hp = _nhwc_rows(h)
        N = conv.weight.shape[0]
        skip = None if skips is None else skips[p]
        out = None if outs is None else outs[p]
        if out is None:
            out = torch.empty((h.shape[0], N) + tuple(h.shape[2:]), dtype=h.dtype, device=h.device, memory_format=torch.channels_last)
            if _nhwc_rows(out) is None:        # (a one-pixel tensor's strides are the allocator's choice: make the rows explicit)
                out = torch.empty((M, N), dtype=h.dtype, device=h.device).view(h.shape[0], h.shape[2], h.shape[3], N).permute(0, 3, 1, 2)
        e = table[p]
        e.h, e.w, e.bias, e.out = h.data_ptr(), conv.weight.data_ptr(), conv.bias.data_ptr(), out.data_ptr()
        e.skip = skip.data_ptr() if skip is not None else None
        e.M, e.N, e.K = M, N, K
        e.h_stride, e.out_stride = hp, _nhwc_rows(out)[2]
        e.skip_stride = _nhwc_rows(skip)[2] if skip is not None else 0
        result.append(out)
    d = _lib.ControlDesc(ctypes.sizeof(_lib.ControlDesc), _DT[hs[0].dtype], n, 0)
    with torch.cuda.device(hs[0].device):
        _lib.check(lib.pww_control_fwd(table, ctypes.byref(d), _ptr(scale_word), _stream()), "pww_control_fwd", lib)
    CONTROL_LAUNCHES[0] += 1
    CONTROL_LAUNCHES[1] += n
    return result
