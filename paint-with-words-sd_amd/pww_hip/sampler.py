"""Denoising driver around the HIP attention path (reference loop: paint_with_words/paint_with_words.py
:431-506; inpaint variant paint_with_words_inpaint.py:230-266).

Three execution modes over the SAME arithmetic:
  "eager"   two batch-1 UNet calls per step (cond dict, then uncond dict), exactly the reference's
            call pattern (:483-499) -- the parity mode.
  "folded"  cond and uncond rows of all images in ONE UNet call ([cond rows..., uncond rows...]); the
            PwW bias is gated per row by the `_PWW_ROW_GATE` coefficients (kernel arg bias_coeff), and
            the qk reductions stay per image (QKProxy).
  "graph"   "folded", with the UNet call captured ONCE into a hipGraph (torch.cuda.CUDAGraph on ROCm) and
            replayed for every step of every request of the same geometry: at batch 1 the UNet is
            launch-bound (~1.5k kernels per call), so replay removes the host launch cost. The only
            step-dependent kernel arguments -- the Python scalars c0 * g(sigma) the user's
            weight_function produces -- live in device words (attention.CoeffSlots) that the host
            rewrites before each replay. A weight function that is not of the form
            c * w * reduce(qk) bakes sigma into torch ops; the sampler then keeps one graph per step.
LoRA adapters (pww_hip/lora.py) are chosen per row by two device arrays of the UNet's LoraState, written in place here: once per request in
"folded" / "graph" (before the K|V projections are refreshed: they are adapted too), before every batch-1 call in "eager".
Region prompts (a full prompt per colour, `regions=`) add K rows per image in each of the three: K more batch-1 calls in "eager", rows
[base x n, region 1 x n, ..., region K x n, uncond x n] in "folded" / "graph" (_fold_regions), and the per-pixel blend of
ops.region_combine where classifier-free guidance is combined otherwise.
A canvas larger than the UNet's window (`canvas=`, MultiDiffusion) is denoised as overlapping windows: the windows are the images of the UNet
evaluation -- one context dict, one region plan, one LoRA row per window -- around two launches per step: ops.canvas_gather forms the windows'
rows from the fp32 canvas latent, ops.canvas_combine the canvas-sized noise prediction from the UNet's output, and one scheduler.step follows
on the canvas.
Region strength (`hold=`, img2img; Differential Diffusion): every latent pixel has a strength S in [0, 1] and is released to the loop at the
step its strength allows (hold_thresholds); one launch behind every scheduler.step (ops.hold_apply, outside the captured graph) puts the
pixels that the next step does not release back to the init latent noised to that step's timestep.
ControlNets (`control=`, a controlnet.ControlRequest): every evaluation of the UNet goes through a controlnet.ControlledUNet instead -- the
ControlNet's encoder on the same rows, then one grouped launch per net that scales its thirteen zero convolutions and adds them into the UNet's
skip tensors. The hint (the embedded control image) lives in a static tensor, one row per UNet row; the conditioning scale in a device word
that is rewritten before every evaluation: 0 outside the guidance window, where "eager" and "folded" skip the ControlNet and "graph" replays
its ONE graph with the word at 0.
Euler, Euler ancestral, DDIM and DPM-Solver++(2M) (pww_hip/steps.py: the schedulers `steps.covers` knows) take every step as ONE launch
(ops.sched_step, outside the captured graph): the guidance combine, the scheduler's update as seven numbers, the history write and the next
UNet input -- written straight into the graph's static input in "graph" -- where LMS and PLMS keep ops.cfg_combine + scheduler.step +
scale_model_input + cat + cast, launch for launch. The plan is built once per request and the history tensor kept here; the scheduler
object's state is not advanced. PWW_STEP=0 keeps scheduler.step everywhere.
"""
import numpy as np
import torch

from . import ops
from . import attnmaps
from . import lora as _lora
from . import controlnet as _controlnet
from . import steps as _steps
from .attention import install, refresh_kv_cache, refresh_orig_cache, ROW_GATE, KV_CACHE, COEFF_SLOTS, CoeffSlots, COMPACT_W, COMPACT_IDX, GATED_ROWS, COND_ROWS, BIAS_COLS, ATTN_RECORDER
from .conditioning import PwWContext

ORIG = "CROSS_ATTENTION_WEIGHT_ORIG"


def _orig_pending(d):
    return isinstance(d, PwWContext) and d.pending(ORIG)


def initial_latents(seed, in_channels, height, width, region_masks=None, extra_seeds=None, batch_seeds=None):
    """:445-455. CPU generator, exactly as the reference, so results do not depend on the device or
    the number of GPUs. `region_masks`: callable(dtype, size) -> list of [1,1,h,w] masks for the seeded
    regions (the reference's _get_binary_mask). `batch_seeds`: one latent per seed (batched mode)."""
    seeds = [seed] if batch_seeds is None else list(batch_seeds)
    size = (1, in_channels, height // 8, width // 8)
    out = []
    for s in seeds:
        latents = torch.randn(size, generator=torch.manual_seed(s))
        if extra_seeds:
            print("Use region based seeding: ", extra_seeds)
            multi = [torch.randn(size, generator=torch.manual_seed(_s)) for _s in extra_seeds.values()]
            masks = region_masks(latents[0].dtype, size[-2:])
            foreground = (sum(masks) > 0).squeeze()
            summed = sum(l * m for l, m in zip(multi, masks))
            latents[:, :, foreground] = summed[:, :, foreground]
        out.append(latents)
    return torch.cat(out, dim=0)


def canvas_plan(canvas_hw, window, stride, ramp=0):
    """The plan `PwWSampler.sample(canvas=)` takes, in latent pixels: canvas_hw = (Hc, Wc), a square window of `window`, origins every
    `stride` with the last window clamped to the end (ops.canvas_windows), `ramp` the length of the linear weight ramp at a window's edges
    (0: every covering window counts the same). Window iy * nx + ix has its origin at (ys[iy], xs[ix])."""
    Hc, Wc = (int(v) for v in canvas_hw)
    return {"size": (Hc, Wc), "window": (int(window), int(window)), "ys": ops.canvas_windows(Hc, window, stride),
            "xs": ops.canvas_windows(Wc, window, stride), "ramp": int(ramp)}


def hold_thresholds(T):
    """theta_g = fp32((T - g) / T) for g = 0 .. T, the quotient formed in double: a pixel of strength S is released at step g of a T-step
    schedule iff fp32(S) >= theta_g (equality releases). A list of T + 1 Python floats that are exact fp32 values (pww_hold_thresholds of
    include/pww_hip_hold.h)."""
    T = int(T)
    if T < 1:
        raise ValueError("hold_thresholds: %d steps" % T)
    return [float(np.float32((T - g) / T)) for g in range(T + 1)]


def hold_first(T, strength):
    """first(s): the smallest step g of a T-step schedule with fp32(s) >= theta_g -- the step at which a pixel of that strength is released,
    and, for the largest strength of a request, the first step the request runs. T when s is below every theta but theta_T = 0 (nothing
    would be denoised)."""
    s = np.float32(strength)
    if not 0.0 <= s <= 1.0:
        raise ValueError("hold_first: strength %r outside [0, 1]" % (strength,))
    for g, theta in enumerate(hold_thresholds(T)):
        if s >= np.float32(theta):
            return g
    raise AssertionError("theta_T is 0")


def _as_list(x, n):
    """One context dict per image: a single dict serves every image of the batch."""
    if isinstance(x, (list, tuple)):
        if len(x) not in (1, n):
            raise ValueError("got %d context dicts for %d images" % (len(x), n))
        return list(x) if len(x) == n else [x[0]] * n
    return [x] * n


def _has_negative_maps(d):
    """Does an unconditional dict carry weight maps of its own (negative regions: conditioning._encode_text_color_inputs with a
    negative_color_context) instead of the reference's integer 0 in every slot?"""
    return any(torch.is_tensor(v) for k, v in dict.items(d) if k.startswith("CROSS_ATTENTION_WEIGHT_")) or _orig_pending(d)


def _fold_negative(conds, unconds, folded, n_images, negative_strength, device):
    """The weight entries of a folded dict whose unconditional rows are biased too (negative regions): every map is materialised as
    [2n, 1, N, T] -- the conditional images' maps, then the unconditional images' -- the gate is [1..., negative_strength...], the column
    bound is taken over both halves, and no image is gated out: the work-distribution hint is 0 while the recorder still learns that the
    first n rows are the conditional ones."""
    folded[ROW_GATE] = torch.cat([torch.ones(n_images), torch.full((n_images,), float(negative_strength))]).to(device=device, dtype=torch.float32)
    folded[GATED_ROWS] = 0
    folded[COND_ROWS] = n_images
    for key in [k for k in list(folded) if k.startswith(COMPACT_W) or k == COMPACT_IDX]:      # (the opt-in compact form is the conditional side's alone)
        folded.pop(key)
    if any(_orig_pending(d) or torch.is_tensor(dict.get(d, ORIG)) for d in conds + unconds):
        def stacked_orig(conds=conds, unconds=unconds):
            w = [d[ORIG] for d in conds + unconds]
            if not all(torch.is_tensor(m) for m in w):
                raise ValueError("negative regions: every context must carry a tensor for %s" % ORIG)
            return torch.stack(w, dim=0)                         # [2n, H, W, T]
        folded.pop(ORIG, None)
        folded.set_lazy(ORIG, stacked_orig)
    for key in [k for k in dict.keys(conds[0]) if k.startswith("CROSS_ATTENTION_WEIGHT_") and k != ORIG]:
        maps = [d.get(key) for d in conds + unconds]
        if not all(torch.is_tensor(m) for m in maps):
            raise ValueError("negative regions: every context must carry a tensor for %s" % key)
        if len({tuple(m.shape) for m in maps}) != 1:
            raise ValueError("negative regions: %s has shapes %s (prompt and unconditional prompt must be encoded to the same number of chunks)"
                             % (key, sorted({tuple(m.shape) for m in maps})))
        folded[key] = torch.stack(maps, dim=0).unsqueeze(1)      # [2n, 1, N, T]
    bounds = [int(d.get(BIAS_COLS, 0) or 0) for d in conds + unconds]
    folded[BIAS_COLS] = max(bounds) if all(bounds) else 0
    return folded


def _context_rows(dicts, n_images):
    """The CONTEXT_TENSOR rows of one row class of a folded call: [n, T, ctx]."""
    if all(d is dicts[0] for d in dicts):
        t = dicts[0]["CONTEXT_TENSOR"]
        return t.expand(n_images, -1, -1) if t.shape[0] == 1 else t
    return torch.cat([d["CONTEXT_TENSOR"] for d in dicts], dim=0)


def _fold_regions(cond, regions, uncond, n_images, device):
    """The single dict of a folded call with region prompts: rows [base x n, region 1 x n, ..., region K x n, uncond x n]. `regions`: one
    plan (conditioning.encode_region_prompts) or one per image, all with the same K. Only the base rows are biased: the gate is ones for the
    first n rows and zeros after, the work-distribution hint is n, and whatever _fold_context stacked per image (weight maps, the
    full-resolution fallback map, the compact forms) is padded with zeros (column index -1) for every row past n."""
    conds, plans = _as_list(cond, n_images), _as_list(regions, n_images)
    K = len(plans[0]["contexts"])
    if K < 1 or any(len(p["contexts"]) != K for p in plans):
        raise ValueError("region prompts: every image of one call must carry the same number of regions (got %s)" % [len(p["contexts"]) for p in plans])
    folded = _fold_context(cond, uncond, n_images, device)
    if folded.get(GATED_ROWS) != n_images:
        raise ValueError("region prompts do not combine with negative regions")
    n, extra = n_images, (K + 1) * n_images
    ct = folded["CONTEXT_TENSOR"]
    region_rows = [_context_rows([p["contexts"][k] for p in plans], n) for k in range(K)]
    shapes = {tuple(r.shape[1:]) for r in region_rows} | {tuple(ct.shape[1:])}
    if len(shapes) != 1:
        raise ValueError("region prompts: every prompt of one call must be encoded to the same number of chunks (got %s)" % sorted(shapes))
    folded["CONTEXT_TENSOR"] = torch.cat([ct[:n]] + region_rows + [ct[n:]], dim=0).contiguous()
    folded[ROW_GATE] = torch.cat([torch.ones(n), torch.zeros(extra)]).to(device=device, dtype=torch.float32)
    if all(c is conds[0] for c in conds):
        return folded                       # shared maps stay [N, T]: the gate keeps them off every row past n

    def pad(t, fill=0):
        return torch.cat([t[:n], t.new_full((extra,) + tuple(t.shape[1:]), fill)], dim=0).contiguous()
    if folded.pending(ORIG):
        stacked = folded._thunks[ORIG]
        folded.set_lazy(ORIG, lambda: pad(stacked()))
    for key in list(dict.keys(folded)):
        v = dict.get(folded, key)
        if not torch.is_tensor(v) or v.shape[0] != 2 * n:
            continue
        if key.startswith("CROSS_ATTENTION_WEIGHT_") and v.dim() == 4:
            folded[key] = pad(v)
        elif key.startswith(COMPACT_W) and v.dim() == 3:
            folded[key] = pad(v)
        elif key == COMPACT_IDX:
            folded[key] = pad(v, -1)
    return folded


def region_blend_fp32(eps, masks, weights, scales, guidance_scale):
    """ops.region_combine's formula on fp32 tensors, operation by operation (include/pww_hip_regions.h): what a UNet that runs in fp32 is
    combined with, as `uncond + g * (cond - uncond)` is without regions."""
    n, K = masks.shape[:2]
    e = eps.float().reshape((K + 2, n) + tuple(eps.shape[1:]))
    u = e[K + 1]
    wk = [weights[:, k, None, None] * masks[:, k] for k in range(K)]            # [n, h, w] each
    total = wk[0]
    for k in range(1, K):
        total = total + wk[k]
    acc = u + ((1.0 - total) * float(guidance_scale))[:, None] * (e[0] - u)
    for k in range(K):
        acc = acc + (wk[k] * scales[:, k, None, None])[:, None] * (e[k + 1] - u)
    return acc


def _fold_context(cond, uncond, n_images, device, negative_strength=1.0):
    """Build the single dict of a folded call: rows [cond x n, uncond x n]. `cond` / `uncond`: one dict, or one dict per
    image (paint_with_words_batch: per-image prompts and color maps). Per-image weight maps are stacked to
    [2n, 1, N, 77] -- the kernels take the image axis through bias_stride[0] -- with zeros for the unconditional rows
    (their gate is 0, the values are never used); a shared map stays [N, 77]. Unconditional dicts with weight maps of their own
    (negative regions) put those maps into the unconditional rows and `negative_strength` into their gate: _fold_negative."""
    conds, unconds = _as_list(cond, n_images), _as_list(uncond, n_images)
    shared = all(c is conds[0] for c in conds)

    def rows(dicts):
        return _context_rows(dicts, n_images)

    folded = conds[0].copy() if isinstance(conds[0], PwWContext) else PwWContext(conds[0])      # (keeps a pending ORIG map pending)
    folded[KV_CACHE] = {}
    folded.pop("_PWW_ORIG_CACHE", None)
    folded["CONTEXT_TENSOR"] = torch.cat([rows(conds), rows(unconds)], dim=0).contiguous()
    folded[ROW_GATE] = torch.cat([torch.ones(n_images), torch.zeros(n_images)]).to(device=device, dtype=torch.float32)
    folded[GATED_ROWS] = n_images        # what the gate holds, for the host side (work distribution of the fused launch)
    if any(_has_negative_maps(u) for u in unconds):
        return _fold_negative(conds, unconds, folded, n_images, negative_strength, device)
    if not shared:
        if any(_orig_pending(c) for c in conds):
            # per-image fallback maps, stacked on first use: [2n, H, W, 77] (zeros for the unconditional rows)
            def stacked_orig(conds=conds):
                w = torch.stack([c[ORIG] for c in conds], dim=0)
                return torch.cat([w, torch.zeros_like(w)], dim=0)
            folded.pop(ORIG, None)
            folded.set_lazy(ORIG, stacked_orig)
        for key in [k for k in dict.keys(conds[0]) if k.startswith("CROSS_ATTENTION_WEIGHT_") and not (k == ORIG and ORIG in folded._thunks)]:
            maps = [c[key] for c in conds]
            if not all(torch.is_tensor(m) for m in maps):
                raise ValueError("per-image contexts must all carry a tensor for %s" % key)
            w = torch.stack(maps, dim=0)                       # [n, N, 77]  (ORIG: [n, H, W, 77])
            w = torch.cat([w, torch.zeros_like(w)], dim=0)
            folded[key] = w if key.endswith("_ORIG") else w.unsqueeze(1)
        # private hints: the column bound is the largest of the images'; the compact forms are padded to one width
        # (unused slots: column index -1) and stacked like the maps
        folded["_PWW_BIAS_COLS"] = max((int(c.get("_PWW_BIAS_COLS", 0) or 0) for c in conds), default=0) if all(c.get("_PWW_BIAS_COLS") for c in conds) else 0
        idxs = [c.get(COMPACT_IDX) for c in conds]
        for key in [k for k in list(folded) if k.startswith(COMPACT_W) or k == COMPACT_IDX]:
            folded.pop(key)
        if all(torch.is_tensor(i) for i in idxs):
            R = max(int(i.numel()) for i in idxs)
            pad_i = [torch.cat([i, i.new_full((R - i.numel(),), -1)]) for i in idxs]
            idx = torch.stack(pad_i + [torch.full_like(pad_i[0], -1)] * n_images, dim=0)          # [2n, R]
            ok = True
            stacked = {}
            for key in [k for k in conds[0] if k.startswith(COMPACT_W)]:
                ws = [c.get(key) for c in conds]
                if not all(torch.is_tensor(w) for w in ws):
                    ok = False
                    break
                ws = [torch.cat([w, w.new_zeros(w.shape[0], R - w.shape[1])], dim=1) for w in ws]
                w = torch.stack(ws, dim=0)                                                         # [n, N, R]
                stacked[key] = torch.cat([w, torch.zeros_like(w)], dim=0).contiguous()
            if ok:
                folded.update(stacked)
                folded[COMPACT_IDX] = idx.contiguous()
    return folded


def weight_function_signature(f):
    """Cache key of the FALL-BACK path only (weight functions that are not c * w * reduce(qk): one hipGraph per step with
    sigma baked into torch ops). What such graphs depend on in the function: its code and every constant it can see --
    closure cells, defaults, the constants of nested code objects (inner lambdas, comprehensions), numeric globals. A function
    that reaches anything else (a non-numeric global such as a helper function or a config object, a closure over a mutable
    object, a callable object) is keyed by a fresh token, i.e. it never matches a cached key and is re-captured: slower, never
    stale. (The regular path needs none of this: the host re-evaluates the function every step, attention.CoeffSlots.)"""
    fresh = ("fresh", object())

    def atom(v):
        if isinstance(v, (int, float, str, bool, bytes, type(None))):
            return ("v", type(v).__name__, v)
        if isinstance(v, tuple) and all(isinstance(x, (int, float, str, bool, type(None))) for x in v):
            return ("t", v)
        return None

    def code_key(code):
        consts = []
        for c in code.co_consts:
            if hasattr(c, "co_code"):
                consts.append(code_key(c))
            else:
                a = atom(c)
                consts.append(a if a is not None else ("repr", repr(c)))     # frozenset / Ellipsis ...: immutable constants
        return ("code", code.co_code, tuple(consts), code.co_names, code.co_varnames[:code.co_argcount])

    def names_of(code):
        out = set(code.co_names)
        for c in code.co_consts:
            if hasattr(c, "co_code"):
                out |= names_of(c)
        return out

    code = getattr(f, "__code__", None)
    if code is None:       # callable object / builtin
        return fresh
    cells = tuple(atom(c.cell_contents) for c in (f.__closure__ or ()))
    dvals = tuple(atom(v) for v in (f.__defaults__ or ()))
    kvals = tuple((k, atom(v)) for k, v in sorted((f.__kwdefaults__ or {}).items()))
    if any(c is None for c in cells) or any(d is None for d in dvals) or any(v is None for _, v in kvals):
        return fresh
    defaults = dvals + kvals
    import types
    g = getattr(f, "__globals__", {})
    globs = []
    for n in sorted(names_of(code)):       # (co_names also holds attribute names -- log, max, std ...: only real globals count)
        if n in g:
            a = atom(g[n])
            if a is None and not isinstance(g[n], types.ModuleType):
                return fresh       # helper function, config object ...: cannot be proven constant
            globs.append((n, a if a is not None else ("module", g[n].__name__)))
    return (code_key(code), cells, defaults, tuple(globs))


class _GraphedUNet:
    """Capture-once / replay-many wrapper of the folded UNet call: key "all" (one graph for every step) while the weight
    function's scalars travel in device words, else one graph per step index."""

    def __init__(self, unet):
        self.unet = unet
        self.graphs = {}
        self.pool = None
        self.static_in = None
        self.static_t = None
        self.captures = 0

    def reset(self):
        """Drop every captured graph AND the memory pool they shared: once the last graph of a pool is gone the
        allocator retires the pool, and capturing into the stale handle trips an internal assert."""
        self.graphs.clear()
        self.pool = None

    def __call__(self, step, x, t_value, context):
        if self.static_in is None or self.static_in.shape != x.shape or self.static_in.dtype != x.dtype:
            self.reset()
            self.static_in = torch.empty_like(x)
            self.static_t = torch.zeros((), dtype=torch.float32, device=x.device)
        if x is not self.static_in:      # (the fused step launch writes the next input into static_in itself)
            self.static_in.copy_(x)
        self.static_t.fill_(float(t_value))
        slots = context.get(COEFF_SLOTS)
        key = "all" if slots is not None and not slots.unsupported else step
        entry = self.graphs.get(key)
        rec = context.get(ATTN_RECORDER)      # attention-map recording: its launches are ordinary nodes of the graph, behind each attention launch
        if entry is None:
            # warm-up on a side stream (required before capture; also the discovery pass of the coefficient slots), then capture
            if slots is not None:
                slots.discover = True
                slots.begin_forward()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            if rec is not None:
                rec.muted = True              # the warm-up pass only allocates the accumulators: what it computes is replayed right below
            try:
                with torch.cuda.stream(s):
                    self.unet(self.static_in, self.static_t, encoder_hidden_states=context)
            finally:
                if rec is not None:
                    rec.muted = False
            torch.cuda.current_stream().wait_stream(s)
            if slots is not None:
                slots.discover = False
                slots.begin_forward()
                key = "all" if not slots.unsupported else step
            g = torch.cuda.CUDAGraph()
            if self.pool is None:
                self.pool = torch.cuda.graph_pool_handle()
            if rec is not None:
                rec.begin_trace()
            try:
                with torch.cuda.graph(g, pool=self.pool):
                    out = self.unet(self.static_in, self.static_t, encoder_hidden_states=context).sample
            finally:
                trace = rec.end_trace() if rec is not None else None
            entry = (g, out, trace)
            self.graphs[key] = entry
            self.captures += 1
        g, out, trace = entry
        g.replay()
        if hasattr(self.unet, "replayed"):
            self.unet.replayed()      # a ControlledUNet's tally of the launches the replay ran again
        if rec is not None and trace:
            rec.replayed(trace)       # the host's tally of what the replay added to each accumulator
        return out


class PwWSampler:
    """Runs the reference's sampling loop for one or many images on one GPU."""

    def __init__(self, unet, scheduler, mode="eager"):
        if mode not in ("eager", "folded", "graph"):
            raise ValueError("mode must be eager | folded | graph")
        self.unet, self.scheduler, self.mode = unet, scheduler, mode
        install(unet)
        self._graphed = _GraphedUNet(unet) if mode == "graph" else None
        self._graph_sig = None
        self._fallback_sig = None
        self._static_folded = None
        self._static_maps = {"bufs": {}, "meta": {}}           # hipGraph mode: the attention-map accumulators the captured probabilities launches add into
        self._request_folded = None
        self._scratch_modules = None
        self._errors = ops.FusedErrorWatch()
        self._lora = None                # the UNet's lora.LoraState while adapters are loaded (looked up per request)
        self._controlled = {}            # (ids of the nets) -> the controlnet.ControlledUNet of this UNet with them
        self._lora_calls = None          # eager mode: the one-row assignment of every batch-1 call of the request, [class * n + image]
        self.handoff_pending = False     # the last request issued launches with an in-kernel hand-off (PWW_QPROJ_STAT=0 / shapes the
                                         # to_q GEMM does not cover): its latents must not reach a caller before check_errors() has looked

    def _static_context(self, folded, weight_function, latents, timesteps, rec=None, batch_shape=None, control=None):
        """Captured graphs read the context tensors by ADDRESS: keep one set of static tensors alive and copy each new
        request's values into them; rebuild the graphs when the geometry changes. The weight function and the schedule are
        NOT part of the key while the function's scalars travel in device words (CoeffSlots) -- fresh lambdas, other
        constants, another step count all replay the same graph; only the per-step fall-back keys them."""
        def tensor_sig(d):      # (the full-resolution fallback map is not part of the geometry: it exists only once a layer asked for it)
            return tuple(sorted((k, tuple(v.shape), v.dtype) for k, v in d.items() if torch.is_tensor(v) and k != ORIG))
        # (a canvas request is keyed on its window batch [n_w, C, h, w] -- what the UNet sees -- not on the canvas or the origins)
        # (recording attention maps on / off, per layer or not, is geometry too: the captured graph holds the probabilities launches or it does not)
        sig = (tuple(latents.shape) if batch_shape is None else tuple(batch_shape), tensor_sig(folded), tuple(sorted((k, v) for k, v in folded.items() if isinstance(v, int) and not isinstance(v, bool))),
               None if rec is None else ("attention maps", rec.per_layer))
        if self._lora is not None:      # LoRA launches are part of the graph: with which padded rank, over which stacks -- not for which rows
            sig = sig + (self._lora.signature(),)
        if control is not None:         # the ControlNets' launches are part of the graph: which nets, the hints' shapes, which route -- not the image, scale or window
            sig = sig + (control.signature(),)
        self._request_folded = folded
        if sig != self._graph_sig:
            self._graphed.reset()
            self._graph_sig = sig
            self._static_maps = {"bufs": {}, "meta": {}}
            self._fallback_sig = None
            self._static_folded = PwWContext({k: (v.clone() if torch.is_tensor(v) else v) for k, v in folded.items() if k != ORIG})
            # CROSS_ATTENTION_WEIGHT_ORIG stays pending in the static context too: the first layer that takes the fallback (in the
            # eager warm-up pass before the capture) clones the CURRENT request's map; later requests copy theirs into it
            self._static_folded.set_lazy(ORIG, lambda: self._request_folded[ORIG].clone())
            self._static_folded[COEFF_SLOTS] = CoeffSlots(latents.device)
        else:
            for k, v in folded.items():
                if torch.is_tensor(v) and k != ORIG:
                    self._static_folded[k].copy_(v)
            if dict.__contains__(self._static_folded, ORIG) and torch.is_tensor(self._static_folded[ORIG]):
                self._static_folded[ORIG].copy_(folded[ORIG])      # (builds this request's map: the captured layers read it)
            refresh_kv_cache(self._static_folded)     # new prompt embedding -> new K|V, same addresses
            refresh_orig_cache(self._static_folded)   # new color map -> new fallback maps, same addresses
        if rec is not None:
            self._static_folded[ATTN_RECORDER] = rec
        else:
            self._static_folded.pop(ATTN_RECORDER, None)
        slots = self._static_folded[COEFF_SLOTS]
        if slots.unsupported:      # one graph per step: those do depend on the function's constants and on the schedule
            fsig = (weight_function_signature(weight_function), tuple(float(t) for t in timesteps))
            if fsig != self._fallback_sig:
                self._graphed.reset()
                self._fallback_sig = fsig
        return self._static_folded

    def _input_scale(self, t, sigma):
        """What scheduler.scale_model_input divides by at timestep t, as one fp32 number (the canvas path divides inside the gather launch):
        1 for a scheduler that hands its input back, sqrt(sigma^2 + 1) formed in fp32 like the LMS scheduler forms it. The scheduler is asked
        with a one-element probe, so one that scales in another way is refused instead of mis-scaled."""
        where = sigma.device if torch.is_tensor(sigma) else "cpu"
        probe = float(self.scheduler.scale_model_input(torch.ones(1, dtype=torch.float32, device=where), t).reshape(-1)[0])
        if probe == 1.0:
            return 1.0
        denom = float((torch.as_tensor(sigma, dtype=torch.float32).cpu() ** 2 + 1) ** 0.5)
        if abs(probe * denom - 1.0) > 1e-5:
            raise ValueError("canvas: the scheduler scales its input by %g at t = %s, which is neither 1 nor 1 / sqrt(sigma^2 + 1) = %g" % (probe, float(t), 1.0 / denom))
        return denom

    def _hold_coefficients(self, t):
        """(a, b) of scheduler.add_noise at timestep t -- add_noise(x0, z, t) = a x0 + b z -- as two fp32 numbers, asked with one-element
        probes like _input_scale asks scale_model_input; a scheduler whose add_noise is not of that form is refused."""
        sch = self.scheduler
        tt = torch.as_tensor(t).reshape(1)
        one, zero = torch.ones(1, dtype=torch.float32), torch.zeros(1, dtype=torch.float32)
        a, b, ab = (float(sch.add_noise(u, v, tt).reshape(-1)[0]) for u, v in ((one, zero), (zero, one), (one, one)))
        if not abs(ab - (a + b)) <= 1e-6:
            raise ValueError("region strength: the scheduler's add_noise is not a x0 + b z at t = %s (add_noise(1, 0) = %g, add_noise(0, 1) = %g, "
                             "add_noise(1, 1) = %g)" % (float(t), a, b, ab))
        return a, b

    def _hold_table(self, hold, latents, timesteps, extra_channels):
        """The `hold` argument of sample() against the request -> one (theta, a, b) per step of `timesteps`: what the launch behind that
        step's scheduler.step holds the latent to. The steps are g = first .. T - 1 of the T-step schedule; behind step g the pixels that
        step g + 1 does not release (S < theta_{g + 1}) go back to add_noise(x0, z, t_{g + 1}); behind the last step the pixels that were
        never released (S < theta_{T - 1}) become x0."""
        if extra_channels is not None:
            raise ValueError("region strength: extra UNet input channels (inpainting) are not supported")
        if not hasattr(self.scheduler, "add_noise"):
            raise ValueError("region strength needs a scheduler with add_noise (%s has none)" % type(self.scheduler).__name__)
        T, first = int(hold["steps"]), int(hold["first"])
        if not 0 <= first < T or len(timesteps) != T - first:
            raise ValueError("region strength: %d timesteps do not go with the steps %d .. %d of a %d-step schedule" % (len(timesteps), first, T - 1, T))
        x0, z, S = hold["init"], hold["noise"], hold["strength"]
        if (latents.dtype != torch.float32 or any(t.dtype != torch.float32 or t.device != latents.device for t in (x0, z, S)) or x0.shape != latents.shape
                or z.shape != latents.shape or tuple(S.shape) != (latents.shape[0],) + tuple(latents.shape[2:])):
            raise ValueError("region strength: the latent is %s %s; the init latent %s, the noise %s and the strength map %s must be float32 on its "
                             "device, two of its shape and one [n, h, w]" % (tuple(latents.shape), latents.dtype, tuple(x0.shape), tuple(z.shape), tuple(S.shape)))
        theta = hold_thresholds(T)
        table = [(theta[first + i + 1],) + self._hold_coefficients(timesteps[i + 1]) for i in range(T - first - 1)]
        return table + [(theta[T - 1], 1.0, 0.0)]

    def _canvas_check(self, canvas, latents, extra_channels):
        """The plan of a canvas request against its latent -> (n_w, (h, w)). The origins themselves are checked by the library."""
        if extra_channels is not None:
            raise ValueError("canvas: extra UNet input channels (inpainting) are not supported")
        if attnmaps.active() is not None:
            raise ValueError("canvas: record_attention_maps() is not supported with a canvas larger than the window (stitched maps are not built)")
        if latents.dim() != 4 or latents.shape[0] != 1 or latents.dtype != torch.float32:
            raise ValueError("canvas: the latent must be one float32 canvas [1, C, Hc, Wc] (got %s %s)" % (tuple(latents.shape), latents.dtype))
        if tuple(canvas["size"]) != tuple(latents.shape[-2:]):
            raise ValueError("canvas: the plan is for a %s latent but the latent is %s" % (tuple(canvas["size"]), tuple(latents.shape[-2:])))
        udt = self.unet.dtype if hasattr(self.unet, "dtype") else next(self.unet.parameters()).dtype
        if udt not in (torch.float16, torch.bfloat16):
            raise ValueError("canvas: the UNet must run in float16 or bfloat16 (got %s)" % udt)
        return len(canvas["ys"]) * len(canvas["xs"]), tuple(canvas["window"])

    def _sigma_and_index(self, i, t):
        sch = self.scheduler
        ts = sch.timesteps
        # the reference looks the index up by timestep equality (:473); PLMS repeats a timestep, so a
        # scheduler that is not 1:1 falls back to the loop counter (SURVEY.md 8 a-note)
        hits = (ts == t).nonzero()
        idx = int(hits.item()) if hits.numel() == 1 else i
        return sch.sigmas[idx], idx

    @torch.no_grad()
    def sample(self, cond, uncond, latents, timesteps, guidance_scale, weight_function, extra_channels=None,
               on_step=None, negative_strength=1.0, regions=None, lora_rows=None, canvas=None, hold=None, control=None):
        """cond / uncond: the two context dicts of the PwW protocol, or one dict per image (per-image prompts / maps).
        regions: None, or the region prompts of the request -- one plan of conditioning.encode_region_prompts or one per image: K more rows
        per image, blended per latent pixel (ops.region_combine) where guidance is combined otherwise.
        An unconditional dict that carries weight maps (negative regions) is evaluated with `negative_strength * weight_function`.
        lora_rows: None (no row has an adapter), or lora.row_plan's (adapters, scales) for the rows [base x n, region 1 x n, ..., uncond x n].
        latents: [n_images, C, h, w] already scaled by init_noise_sigma (or noised for img2img).
        canvas: None, or a canvas_plan(): `latents` is then ONE float32 canvas [1, C, Hc, Wc] denoised as n_w = ny nx overlapping windows --
        cond / uncond / regions are one per window (or one for all), lora_rows is planned with n = n_w, and every step gathers the windows
        (ops.canvas_gather), evaluates the UNet on (K + 2) n_w rows and combines them into the canvas's noise prediction (ops.canvas_combine)
        for one scheduler.step on the canvas. A weight_function's score statistic (qk.max() ...) is per window, as it is per image. Raises
        ValueError while record_attention_maps() is active, and with extra_channels.
        hold: None, or the region strengths of an img2img request: {"init": x0 and "noise": z, fp32 like `latents` (which is
        add_noise(x0, z, timesteps[0])); "strength": S fp32 [n, h, w] in [0, 1] (ops.hold_strength_map), at canvas size for a canvas
        request; "steps": T, "first": i0 -- `timesteps` are the steps i0 .. T - 1 of the T-step schedule}. Behind every scheduler.step, and in
        front of on_step, one launch (ops.hold_apply; outside the captured graph) holds the pixels the next step does not release.
        control: None, or a controlnet.ControlRequest -- the ControlNets of the request with their control images (one row per image), conditioning
        scales and guidance window. ValueError with a canvas and with extra_channels.
        extra_channels: inpaint's cat([mask, masked_image_latents]) ([n or 1, 5, h, w]) or None."""
        sch, unet, dev = self.scheduler, self.unet, latents.device
        self._errors.poll(wait=False)      # a hand-off time-out of an earlier request surfaces here (or in check_errors())
        install(unet)      # the plug is a class-level patch (:193-195): put it back if somebody removed it since __init__
        n, frame = latents.shape[0], tuple(latents.shape[-2:])      # images of the UNet evaluation and their latent size
        if canvas is not None:
            n, frame = self._canvas_check(canvas, latents, extra_channels)
        udt = unet.dtype if hasattr(unet, "dtype") else next(unet.parameters()).dtype
        conds, unconds = _as_list(cond, n), _as_list(uncond, n)
        held = None if hold is None else dict(hold, table=self._hold_table(hold, latents, timesteps, extra_channels))
        blend = None
        if regions is not None:
            if any(_has_negative_maps(u) for u in unconds):
                raise ValueError("region prompts do not combine with negative regions")
            plans = _as_list(regions, n)
            if any(tuple(p["masks"].shape[-2:]) != frame for p in plans):
                raise ValueError("region prompts: the color map gives %s region masks but the latent is %s: the color map must be 8 x the latent's size"
                                 % (sorted({tuple(p["masks"].shape[-2:]) for p in plans}), frame))
            stack = lambda key: torch.stack([p[key] for p in plans], dim=0).to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
            blend = {"plans": plans, "K": len(plans[0]["contexts"]), "masks": stack("masks"), "weights": stack("weights"), "scales": stack("scales")}
        self._lora = _lora.state_of(unet)
        if self._lora is not None and not self._lora.adapters:
            self._lora = None
        self._lora_calls = None
        if self._lora is None and lora_rows is not None:
            raise ValueError("lora_rows without a loaded LoRA adapter")
        if self._lora is not None:
            rows = ((blend["K"] if blend else 0) + 2) * n
            adapters, scales = lora_rows if lora_rows is not None else ([-1] * rows, [0.0] * rows)
            if len(adapters) != rows or len(scales) != rows:
                raise ValueError("lora_rows: %d adapters / %d scales for %d rows" % (len(adapters), len(scales), rows))
            if self.mode == "eager":
                self._lora_calls = [self._lora.device_rows([a], [s]) for a, s in zip(adapters, scales)]
            else:       # (before _static_context: it refreshes the cached K|V projections, which are adapted per row)
                self._lora.assign(self._lora.device_rows(adapters, scales))
        if self.mode == "eager":   # per-request caches of the fused K|V projections (prompt constant over the steps)
            for d in conds + unconds + ([c for p in blend["plans"] for c in p["contexts"]] if blend else []):
                d.setdefault(KV_CACHE, {}).clear()
        folded = None
        rec = attnmaps.active()        # pww_hip.record_attention_maps(): the recorder rides in the conditional context(s) of this request
        model = None
        if control is not None:
            if canvas is not None:
                raise ValueError("controlnet: a canvas larger than the window is not supported (the hint would have to be cropped per window)")
            if extra_channels is not None:
                raise ValueError("controlnet: extra UNet input channels (inpainting) are not supported")
            key = tuple(id(net) for net in control.nets)
            model = self._controlled.get(key)
            if model is None:
                model = self._controlled[key] = _controlnet.ControlledUNet(unet, control.nets)
            # (before _static_context: the hints' shapes are part of the graph signature)
            model.begin_request(control, n, 1 if self.mode == "eager" else (blend["K"] if blend else 0) + 2)
        if self._graphed is not None:
            self._graphed.unet = unet if model is None else model      # (what the next capture records; the signature below tells them apart)
        more = {} if model is None else {"control": (control, model)}      # (a call without ControlNets is, argument for argument, the call of before)
        if self.mode != "eager":
            folded = _fold_context(cond, uncond, n, dev, negative_strength) if blend is None else _fold_regions(cond, regions, uncond, n, dev)
            if self._graphed is not None:
                if model is not None:
                    folded = self._static_context(folded, weight_function, latents, timesteps, rec, control=model)
                elif canvas is None:
                    folded = self._static_context(folded, weight_function, latents, timesteps, rec)
                else:
                    folded = self._static_context(folded, weight_function, latents, timesteps, rec, batch_shape=(n, latents.shape[1]) + frame)
        if extra_channels is not None and extra_channels.shape[0] != n:
            extra_channels = extra_channels.expand(n, -1, -1, -1)
        if canvas is not None:
            return self._denoise(conds, unconds, folded, latents, timesteps, guidance_scale, weight_function, None, on_step, None, negative_strength, blend, canvas,
                                 hold=held)
        if rec is None:
            return self._denoise(conds, unconds, folded, latents, timesteps, guidance_scale, weight_function, extra_channels, on_step, None, negative_strength, blend,
                                 hold=held, **more)
        static = self._static_maps if self._graphed is not None else None
        rec.begin_request(n, latents.shape[-2:], static=static)      # (hipGraph mode: zeroes the static accumulators, before the first replay)
        holders = conds if folded is None else [folded]
        for d in holders:
            d[ATTN_RECORDER] = rec
        try:
            return self._denoise(conds, unconds, folded, latents, timesteps, guidance_scale, weight_function, extra_channels, on_step, rec, negative_strength, blend,
                                 hold=held, **more)
        finally:
            for d in holders:
                d.pop(ATTN_RECORDER, None)
            rec.end_request(static=static is not None)

    def _denoise(self, conds, unconds, folded, latents, timesteps, guidance_scale, weight_function, extra_channels, on_step, rec, negative_strength=1.0, blend=None,
                 canvas=None, hold=None, control=None):
        """The loop of sample() (reference :470-506). control: None, or (the request, its ControlledUNet). blend: the region prompts of the request (sample()), or None. canvas: the plan of a
        canvas request, or None -- `latents` is then the canvas, and the n images of the UNet evaluation are its windows. hold: the region
        strengths of the request with their (theta, a, b) per step (_hold_table), or None."""
        sch, unet, n = self.scheduler, self.unet, latents.shape[0] if canvas is None else len(conds)
        udt = unet.dtype if hasattr(unet, "dtype") else next(unet.parameters()).dtype
        zero_function = lambda w, sigma, qk: 0.0      # noqa: E731  (the reference's unconditional pass, :493)
        ns = float(negative_strength)
        negative_function = lambda w, sigma, qk: ns * weight_function(w, sigma, qk)      # noqa: E731
        # eager mode: per image, what its unconditional dict is evaluated with (one with weight maps of its own: negative regions)
        uncond_functions = [negative_function if _has_negative_maps(u) else zero_function for u in unconds] if folded is None else None
        K = blend["K"] if blend is not None else 0
        calls = self._lora_calls        # eager mode with LoRA adapters loaded: every batch-1 call has its own one-row assignment
        plain_unet = unet
        # the schedulers steps.covers knows: one launch per step (ops.sched_step) instead of cfg_combine + scheduler.step + the next step's
        # scale_model_input + cat + cast. `fused`: the rows of the request, the history tensor where a row reads it, and u, the next UNet
        # input -- not for canvas, region-strength and inpainting requests, which make their input as before
        fused = None
        if _steps.route(sch, latents):
            rows = _steps.plan(sch, timesteps)
            latents = latents.clone()      # the launch writes in place: the caller's tensor stays what it was, as with scheduler.step
            fused = {"rows": rows, "draws": _steps.stochastic(sch), "u": None,
                     "h": torch.empty(latents.shape, dtype=torch.float32, device=latents.device) if any(r[4] != 0.0 for r in rows) else None,
                     "feeds": (canvas is None and hold is None and extra_channels is None and latents.is_contiguous()
                               and udt in (torch.float16, torch.bfloat16))}      # (an fp32 UNet takes the launch without u, too)
        for i, t in enumerate(timesteps):
            sigma, _ = self._sigma_and_index(i, t)
            if control is not None:
                # the scale words of this step: 0 outside the guidance window. "graph" replays its one graph with them; "eager" and "folded"
                # run the ControlNets only where a word is not 0
                words = control[0].words(i, len(timesteps))
                live = any(w != 0.0 for w in words)
                if self.mode == "graph" or live:
                    control[1].set_words(words)
                unet = control[1] if live else plain_unet
                if not live and self.mode != "graph":
                    _controlnet._STATS["skipped_steps"] += 1
            x2 = None
            if fused is not None and fused["u"] is not None:
                x = x2 = fused["u"]      # the last launch's u: scaled, rounded to the UNet's type, one replica per row class
            elif canvas is None:
                x = sch.scale_model_input(latents, t)
            else:
                # the windows' rows, scaled and rounded to the UNet's type by one launch: [n_w, C, h, w] for the batch-1 calls of "eager",
                # the K + 2 row classes of the folded call otherwise; outside the captured graph in hipGraph mode
                x = ops.canvas_gather(latents, canvas["ys"], canvas["xs"], canvas["window"][0], canvas["window"][1], self._input_scale(t, sigma),
                                      1 if self.mode == "eager" else K + 2, udt)
            if extra_channels is not None:
                x = torch.cat([x, extra_channels.to(x.dtype)], dim=1)
            if self.mode == "eager":
                eps_c, eps_u, eps_r = [], [], [[] for _ in range(K)]
                for j in range(n):   # the reference is batch-1 (:445); images are independent
                    conds[j].update({"SIGMA": sigma, "WEIGHT_FUNCTION": weight_function})
                    if rec is not None:
                        rec.row = j
                    if control is not None:
                        control[1].row = j      # the hint of a batch-1 call is its image's
                    if calls is not None:
                        self._lora_call(calls[j], conds[j], n)
                    eps_c.append(unet(x[j:j + 1], t, encoder_hidden_states=conds[j]).sample)
                    for k in range(K):     # the region prompts: plain cross-attention, like the unconditional pass
                        ctx = blend["plans"][j]["contexts"][k]
                        ctx.update({"SIGMA": sigma, "WEIGHT_FUNCTION": zero_function})
                        if calls is not None:
                            self._lora_call(calls[(k + 1) * n + j], ctx, n)
                        eps_r[k].append(unet(x[j:j + 1], t, encoder_hidden_states=ctx).sample)
                    unconds[j].update({"SIGMA": sigma, "WEIGHT_FUNCTION": uncond_functions[j]})
                    if calls is not None:
                        self._lora_call(calls[(K + 1) * n + j], unconds[j], n)
                    eps_u.append(unet(x[j:j + 1], t, encoder_hidden_states=unconds[j]).sample)
                eps_c, eps_u = torch.cat(eps_c), torch.cat(eps_u)
                out = torch.cat([eps_c] + [torch.cat(r) for r in eps_r] + [eps_u]) if K or canvas is not None else None
            else:
                folded.update({"SIGMA": sigma, "WEIGHT_FUNCTION": weight_function})
                if x2 is None:
                    x2 = torch.cat([x] * (K + 2), dim=0).to(udt) if canvas is None else x
                if self.mode == "graph":
                    slots = folded[COEFF_SLOTS]
                    if not slots.unsupported and not slots.update(weight_function, sigma):
                        # the function changed its structure (another statistic, not symbolic any more): capture again
                        self._graphed.reset()
                        slots.reset()
                    out = self._graphed(i, x2, float(t), folded)
                else:
                    out = unet(x2, t, encoder_hidden_states=folded).sample
                eps_c, eps_u = out[:n], out[n:]
            if canvas is not None:
                # rows [base x n_w, region 1 x n_w, ..., uncond x n_w] -> the canvas's fp32 [1, C, Hc, Wc], one launch (outside the graph too)
                more = {} if not K else {"masks": blend["masks"], "weights": blend["weights"], "scales": blend["scales"]}
                noise_pred = ops.canvas_combine(out, canvas["ys"], canvas["xs"], canvas["size"], guidance_scale, canvas["ramp"], **more)
            elif K:
                # rows [base x n, region 1 x n, ..., uncond x n] -> fp32 [n, C, h, w], one launch; outside the captured graph in hipGraph mode
                combine = ops.region_combine if out.dtype in (torch.float16, torch.bfloat16) else region_blend_fp32
                noise_pred = combine(out, blend["masks"], blend["weights"], blend["scales"], guidance_scale)
            elif eps_c.dtype in (torch.float16, torch.bfloat16):
                # (the fused step launch combines the pair itself)
                noise_pred = (eps_c, eps_u) if fused is not None else ops.cfg_combine(eps_c, eps_u, guidance_scale)     # fp32, :501-503
            else:
                noise_pred = eps_u + guidance_scale * (eps_c - eps_u)
            if fused is None:
                latents = sch.step(noise_pred, t, latents).prev_sample
            else:
                latents = self._fused_step(fused, i, len(timesteps), noise_pred, guidance_scale, latents, (K + 2) if self.mode != "eager" else 1, udt)
            if hold is not None:
                # the pixels the next step does not release go back to the init latent at that step's noise level: one launch, in place, outside
                # the captured graph in hipGraph mode
                theta, a, b = hold["table"][i]
                if latents.is_contiguous():
                    ops.hold_apply(latents, hold["init"], hold["noise"], hold["strength"], theta, a, b)
                else:
                    # (an img2img latent inherits channels_last strides from the VAE's convolution and keeps them: the UNet's stock
                    # convolutions round differently per memory layout, and a request whose strengths hold nothing is the plain call bit
                    # for bit. The launch reads and writes NCHW memory, so such a latent goes through an NCHW copy and back.)
                    latents.copy_(ops.hold_apply(latents.contiguous(), hold["init"], hold["noise"], hold["strength"], theta, a, b))
            if on_step is not None:
                on_step(i, t, latents if fused is None else latents.clone())      # (the next launch overwrites the latent: a callback may keep what it is handed)
        # did any fused cross-attention launch of this request time out in its hand-off? One 4-byte device -> host copy behind an
        # event (ops.FusedErrorWatch): looked at when the next request starts and by check_errors() -- never a host stall here
        if self._scratch_modules is None:
            self._scratch_modules = [m for m in self.unet.modules() if m.__class__.__name__ in ("CrossAttention", "Attention")]
        self.handoff_pending = self._errors.post(self._scratch_modules)
        return latents

    def _fused_step(self, fused, i, T, model, guidance_scale, latents, copies, udt):
        """Step i of T of a request on the fused route: ONE ops.sched_step, in place on the latent (outside the captured graph in hipGraph
        mode, as the hold launch is). model: the (cond, uncond) pair of the UNet's type, or the fp32 blend of a region-prompt / canvas
        request. A stochastic scheduler's noise is drawn here with the one torch.randn call its own step() makes, in the same place of the
        loop, so both routes see the same noise under one seed. The next UNet input goes into fused["u"]: the graph's static input once it
        exists, else a buffer of this request; not behind the last step, and not for requests that make their input as before."""
        z = torch.randn(latents.shape, dtype=torch.float32, device=latents.device) if fused["draws"] else None
        if isinstance(model, tuple):
            model = tuple(m if m.is_contiguous() else m.contiguous() for m in model)
        elif not model.is_contiguous():
            model = model.contiguous()
        u = None
        if fused["feeds"] and i + 1 < T:
            shape = (copies * latents.shape[0],) + tuple(latents.shape[1:])
            static = self._graphed.static_in if self._graphed is not None else None
            if static is not None and tuple(static.shape) == shape and static.dtype == udt and static.is_contiguous():
                u = static
            else:
                u = fused["u"] if fused["u"] is not None and fused["u"] is not static else torch.empty(shape, dtype=udt, device=latents.device)
        fused["u"] = u
        if latents.is_contiguous():
            return ops.sched_step(latents, fused["rows"][i], model, guidance_scale, h=fused["h"], z=z, u=u)
        # (an img2img latent may carry channels_last strides and keeps them, as in the hold launch below: the step runs on an NCHW copy)
        latents.copy_(ops.sched_step(latents.contiguous(), fused["rows"][i], model, guidance_scale, h=fused["h"], z=z))
        return latents

    def _lora_call(self, rows, context, n):
        """Eager mode: the one-row assignment of the batch-1 call about to be made. The dict's cached K|V projection is adapted with the
        row's adapter; a dict that serves several images (each with its own assignment) forms it again per call."""
        self._lora.assign(rows)
        if n > 1:
            context.get(KV_CACHE, {}).clear()

    def check_errors(self):
        """Wait for the requests issued so far and raise PwwHipError if a fused cross-attention hand-off of any of them timed out
        (their outputs are NaN). The PIL-returning entry points call this after decoding; the latent-returning ones
        (`return_latents=True`) call `checked()`."""
        self._errors.poll(wait=True)
        self.handoff_pending = False

    def checked(self, latents):
        """`latents` of the request just issued, safe to hand to a caller: if that request contained launches with an in-kernel
        hand-off (the only launches that can fail at run time) this waits for it and raises on a time-out -- a single call never
        hands back NaN latents silently. The default path (statistic formed in the to_q GEMM, no hand-off) has nothing to wait
        for and stays asynchronous."""
        if self.handoff_pending:
            self.check_errors()
        return latents
