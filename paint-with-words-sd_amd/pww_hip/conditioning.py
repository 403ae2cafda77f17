"""Conditioning builder: color map + color_context + prompt -> the two encoder_hidden_states dicts of
the PwW protocol (reference paint_with_words/paint_with_words.py:207-388), with the per-resolution
token weight maps produced ON DEVICE by pww_mask_build instead of the reference's Python loops over
F.interpolate (:247-276).

Host side (strings, token matching, the region table) stays Python, as in the reference; function
names follow the reference's so the call sites read the same.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F  # noqa: F401  (region-seed masks: _get_binary_mask)

import os

from . import ops

COMPACT_BIAS = os.environ.get("PWW_COMPACT_BIAS", "0") == "1"   # see prepare_conditioning: private compact weight maps, opt-in


class PwWContext(dict):
    """The encoder_hidden_states dict of the PwW protocol (:370-386) with entries that are BUILT ON FIRST ACCESS.

    `CROSS_ATTENTION_WEIGHT_ORIG` (:343-345) is 80.7 MB at 512 x 512 and is only ever read on inj_forward's KeyError path
    (:95-101: a layer whose token count has no per-resolution map -- image sizes that are not multiples of 64, a latent sized
    differently from the color map). The reference builds it for every request; here `context["CROSS_ATTENTION_WEIGHT_ORIG"]`
    runs the mask kernel at ratio 1 the first time somebody asks (dict.__missing__), so requests that never take the fallback
    never pay for it, and code that indexes the dict the way the reference does sees no difference. `in`, `.get()` and `.copy()`
    know about the pending entries; `dict(ctx)` / `.items()` see only what has been built."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._thunks = {}

    def set_lazy(self, key, thunk):
        self._thunks[key] = thunk
        return self

    def pending(self, key):
        return key in self._thunks and not dict.__contains__(self, key)

    def __missing__(self, key):
        thunk = self._thunks.get(key)
        if thunk is None:
            raise KeyError(key)
        value = thunk()
        self[key] = value
        return value

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._thunks

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default

    def copy(self):
        c = PwWContext(self)
        c._thunks = dict(self._thunks)
        return c


def always_round(x):
    """:18-26 (round half up for the non-negative sizes it is applied to)."""
    intx = int(x)
    if intx % 2 == 0:
        return intx if x < intx + 0.5 else intx + 1
    return round(x)


def _extract_seed_and_sigma_from_context(color_context, ignore_seed=-1):
    """:279-297: "text,strength[,seed[,sigma]]" -> strip the tail; mutates `color_context` like the
    reference does (:296). Returns (color_context, {ordinal: seed}, {ordinal: sigma})."""
    extra_seeds, extra_sigmas = {}, {}
    for i, (k, ctx) in enumerate(color_context.items()):
        parts = ctx.split(",")
        if len(parts) > 2:
            try:
                seed = int(parts[-2])
                sigma = float(parts[-1])
                parts = parts[:-2]
                extra_sigmas[i] = sigma
            except ValueError:
                seed = int(parts[-1])
                parts = parts[:-1]
            if seed != ignore_seed:
                extra_seeds[i] = seed
        color_context[k] = ",".join(parts)
    return color_context, extra_seeds, extra_sigmas


def check_negative_context(negative_color_context, negative_strength=1.0):
    """The `negative_color_context` / `negative_strength` keywords of the entry points, checked without touching the caller's dict(s): the
    grammar of color_context, except that a region seed other than -1 is refused -- region seeding belongs to the initial latent, which the
    unconditional side does not own."""
    if isinstance(negative_strength, bool) or not isinstance(negative_strength, (int, float)) or not math.isfinite(float(negative_strength)):
        raise ValueError("negative_strength must be a finite number (got %r)" % (negative_strength,))
    if negative_color_context is None:
        return
    ctxs = negative_color_context if isinstance(negative_color_context, (list, tuple)) else [negative_color_context]
    for ctx in ctxs:
        if ctx is None:
            continue
        _, seeds, _ = _extract_seed_and_sigma_from_context(dict(ctx))
        if seeds:
            raise ValueError("negative_color_context: a region seed (%s) is not supported on the negative side; write -1, as in "
                             "\"phrase,strength,-1,sigma\"" % ", ".join(str(v) for v in seeds.values()))


MAX_REGION_PROMPTS = 8       # region prompts per request (PWW_REGIONS_MAX of include/pww_hip_regions.h)
MAX_REGION_FEATHER = 8.0     # sigma of the feather of the region masks, in latent pixels (PWW_REGIONS_MAX_FEATHER)


def _rgb_of(color):
    """(r, g, b) of a key of color_context / region_prompts: a tuple of three 8-bit ints, or "#rrggbb"."""
    if isinstance(color, str):
        if len(color) != 7 or color[0] != "#":
            raise ValueError("region_prompts: colour %r is not (r, g, b) or \"#rrggbb\"" % (color,))
        try:
            return tuple(int(color[i:i + 2], 16) for i in (1, 3, 5))
        except ValueError:
            raise ValueError("region_prompts: colour %r is not (r, g, b) or \"#rrggbb\"" % (color,))
    if (not isinstance(color, (tuple, list)) or len(color) != 3
            or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) <= 255 for c in color)):
        raise ValueError("region_prompts: colour %r is not (r, g, b) with 8-bit values or \"#rrggbb\"" % (color,))
    return tuple(int(c) for c in color)


def _number(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
        raise ValueError("%s must be a finite number (got %r)" % (name, v))
    return float(v)


def region_entries(region_prompts):
    """One request's `region_prompts` dict -> [((r, g, b), prompt, weight, guidance_scale or None)], checked: 1 .. MAX_REGION_PROMPTS
    entries {colour: "full prompt"} or {colour: ("full prompt", weight in (0, 1], guidance_scale or None)}, no colour twice."""
    if not isinstance(region_prompts, dict):
        raise ValueError("region_prompts must be a dict {(r, g, b): \"prompt\"} or {(r, g, b): (\"prompt\", weight, guidance_scale)} (got %r)"
                         % type(region_prompts).__name__)
    if not 1 <= len(region_prompts) <= MAX_REGION_PROMPTS:
        raise ValueError("region_prompts takes 1 to %d regions (got %d)" % (MAX_REGION_PROMPTS, len(region_prompts)))
    out = []
    for color, value in region_prompts.items():
        rgb = _rgb_of(color)
        if rgb in [e[0] for e in out]:
            raise ValueError("region_prompts names colour %s twice" % (rgb,))
        fields = (value,) if isinstance(value, str) else value
        if not isinstance(fields, (tuple, list)) or not 1 <= len(fields) <= 3 or not isinstance(fields[0], str):
            raise ValueError("region_prompts[%s] must be a prompt or (prompt, weight, guidance_scale) (got %r)" % (rgb, value))
        weight = _number(fields[1], "region_prompts[%s]: weight" % (rgb,)) if len(fields) > 1 else 1.0
        if not 0.0 < weight <= 1.0:
            raise ValueError("region_prompts[%s]: weight must be in (0, 1] (got %r)" % (rgb, weight))
        scale = fields[2] if len(fields) > 2 else None
        if scale is not None:
            scale = _number(scale, "region_prompts[%s]: guidance_scale" % (rgb,))
        out.append((rgb, fields[0], weight, scale))
    return out


def check_region_prompts(region_prompts, region_base_weight=0.0, region_feather=0.0, negative_color_context=None, n_requests=None):
    """The `region_prompts` / `region_base_weight` / `region_feather` keywords of the entry points, checked before any model is touched.
    region_prompts: None or {} (off), one dict (region_entries), or -- the batch forms, `n_requests` given -- a sequence with one dict (or
    None) per request; every request of one call carries the same number of regions. Together with a non-empty negative_color_context it is
    refused. Returns the number of regions per request (0: off)."""
    beta = _number(region_base_weight, "region_base_weight")
    if not 0.0 <= beta < 1.0:
        raise ValueError("region_base_weight must be in [0, 1) (got %r)" % (region_base_weight,))
    feather = _number(region_feather, "region_feather")
    if not 0.0 <= feather <= MAX_REGION_FEATHER:
        raise ValueError("region_feather must be in [0, %g] latent pixels (got %r)" % (MAX_REGION_FEATHER, region_feather))
    if region_prompts is None:
        return 0
    if isinstance(region_prompts, (list, tuple)):
        if n_requests is None:
            raise ValueError("region_prompts must be a dict (a sequence of dicts is the batch form)")
        if len(region_prompts) != n_requests:
            raise ValueError("region_prompts has %d entries for %d requests" % (len(region_prompts), n_requests))
        per = list(region_prompts)
    else:
        per = [region_prompts]
    counts = [0 if r is None or (isinstance(r, dict) and not r) else len(region_entries(r)) for r in per]
    if len(set(counts)) > 1:
        raise ValueError("region_prompts: every request of one call must carry the same number of regions (got %s)" % counts)
    if counts and counts[0]:
        negs = negative_color_context if isinstance(negative_color_context, (list, tuple)) else [negative_color_context]
        if any(negs):
            raise ValueError("region_prompts together with a negative_color_context is not supported")
    return counts[0] if counts else 0


MAX_REGION_STRENGTHS = 8             # named colours per request (PWW_HOLD_MAX_COLORS of include/pww_hip_hold.h)
MAX_REGION_STRENGTH_FEATHER = 8.0    # sigma of the feather of the strength map, in latent pixels (PWW_HOLD_MAX_FEATHER)


def region_strength_entries(region_strength):
    """One request's `region_strength` dict -> [((r, g, b), strength)], checked: 1 .. MAX_REGION_STRENGTHS entries {colour: strength}, the
    colours in the grammar of region_prompts ((r, g, b) or "#rrggbb"), no colour twice, every strength a finite number in [0, 1]."""
    if not isinstance(region_strength, dict):
        raise ValueError("region_strength must be a dict {(r, g, b): strength} (got %r)" % type(region_strength).__name__)
    if not 1 <= len(region_strength) <= MAX_REGION_STRENGTHS:
        raise ValueError("region_strength takes 1 to %d colours (got %d)" % (MAX_REGION_STRENGTHS, len(region_strength)))
    out = []
    for color, value in region_strength.items():
        try:
            rgb = _rgb_of(color)
        except ValueError as e:
            raise ValueError(str(e).replace("region_prompts", "region_strength"))
        if rgb in [e[0] for e in out]:
            raise ValueError("region_strength names colour %s twice" % (rgb,))
        s = _number(value, "region_strength[%s]" % (rgb,))
        if not 0.0 <= s <= 1.0:
            raise ValueError("region_strength[%s] must be in [0, 1] (got %r)" % (rgb, value))
        out.append((rgb, s))
    return out


def check_region_strength(region_strength, feather=0.0, init_images=None, n_requests=None):
    """The `region_strength` / `region_strength_feather` keywords of the entry points, checked before any model is touched.
    region_strength: None or {} (off), one dict (region_strength_entries), or -- the batch forms, `n_requests` given -- a sequence with one
    dict (or None / {}) per request. feather: a finite number of latent pixels in [0, MAX_REGION_STRENGTH_FEATHER]. Both need an init image
    (`init_images`: whatever the face was given, None when it was given none): a strength per colour says how far a region moves from it.
    -> None when the feature is off, else [per request: [((r, g, b), strength)] or None]."""
    sigma = _number(feather, "region_strength_feather")
    if not 0.0 <= sigma <= MAX_REGION_STRENGTH_FEATHER:
        raise ValueError("region_strength_feather must be in [0, %g] latent pixels (got %r)" % (MAX_REGION_STRENGTH_FEATHER, feather))
    if isinstance(region_strength, (list, tuple)):
        if n_requests is None:
            raise ValueError("region_strength must be a dict (a sequence of dicts is the batch form)")
        if len(region_strength) != n_requests:
            raise ValueError("region_strength has %d entries for %d requests" % (len(region_strength), n_requests))
        per = list(region_strength)
    else:
        per = [region_strength] * (1 if n_requests is None else n_requests)
    entries = [None if r is None or (isinstance(r, dict) and not r) else region_strength_entries(r) for r in per]
    on = any(e is not None for e in entries)
    if init_images is None and (on or sigma != 0.0):
        raise ValueError("region_strength and region_strength_feather need an init image (img2img): the strength says how far a region moves from it")
    return entries if on else None


def check_loras(lora, region_loras, region_prompts=None, n_requests=None, tools=None):
    """The `lora` / `region_loras` keywords of the entry points, checked before any model is touched.
    lora: None, "name" or ("name", scale) -- the adapter of every row without one of its own (the conditional / base row, the unconditional
    row, region rows without an entry). region_loras: None or {} (off), {(r, g, b) | "#rrggbb": "name" | ("name", scale)} whose colours are
    keys of the same request's region_prompts, or -- the batch forms, `n_requests` given -- a sequence with one dict (or None) per request.
    Names are resolved against the UNet of `tools` (the call's preloaded_utils; without one nothing can be loaded). Scales are finite numbers.
    -> None when both are off, else ((name, scale) or None, [per request: {(r, g, b): (name, scale)} or None])."""
    from . import lora as _lora
    loaded = _lora.loras(tools[1]) if tools is not None else []

    def entry(value, what):
        e = _lora.lora_entry(value, what)
        if e[0] not in loaded:
            raise ValueError("%s: LoRA adapter %r is not loaded on the UNet of preloaded_utils (loaded: %s); pww_hip.lora.load_lora(unet, source, name) "
                             "loads one" % (what, e[0], loaded))
        return e
    g = None if lora is None else entry(lora, "lora")
    n = n_requests if n_requests is not None else 1
    if isinstance(region_loras, (list, tuple)):
        if n_requests is None:
            raise ValueError("region_loras must be a dict (a sequence of dicts is the batch form)")
        if len(region_loras) != n_requests:
            raise ValueError("region_loras has %d entries for %d requests" % (len(region_loras), n_requests))
        per = list(region_loras)
    else:
        per = [region_loras] * n
    prompts = list(region_prompts) if isinstance(region_prompts, (list, tuple)) else [region_prompts] * n
    out = []
    for rl, rp in zip(per, prompts):
        if rl is None or (isinstance(rl, dict) and not rl):
            out.append(None)
            continue
        if not isinstance(rl, dict):
            raise ValueError("region_loras must be a dict {(r, g, b): \"name\"} or {(r, g, b): (\"name\", scale)} (got %r)" % type(rl).__name__)
        colors = [e[0] for e in region_entries(rp)] if rp else []
        d = {}
        for color, value in rl.items():
            rgb = _rgb_of(color)
            if rgb in d:
                raise ValueError("region_loras names colour %s twice" % (rgb,))
            if rgb not in colors:
                raise ValueError("region_loras: colour %s is not a key of the request's region_prompts (%s)" % (rgb, colors))
            d[rgb] = entry(value, "region_loras[%s]" % (rgb,))
        out.append(d)
    if g is None and not any(out):
        return None
    return g, out


def _encode_row_list(text_encoder, rows, device):
    """The text encoder over `rows` -- [1, L] id tensors (what the tokenizer returns) or id lists of one length L -- -> R tensors [1, L, C].
    A CLIP text model the native route covers (pww_hip.text_encode: `enabled()` and `covers()`) encodes all of them in ONE forward, and the
    list holds its rows; any other encoder (TinyTextEncoder, fp32, CPU) is called exactly as before -- once per row, in order, with a [1, L]
    batch each -- and the list holds the encoder's OWN outputs, so the call sites hand on the very tensors they handed on before."""
    from . import text_encode
    rows = [r if torch.is_tensor(r) else torch.tensor([r], dtype=torch.long) for r in rows]
    if text_encode.enabled() and text_encode.covers(text_encoder):
        return list(text_encode.encode(text_encoder, torch.cat(rows, dim=0)).split(1, dim=0))
    return [text_encoder(r.to(device))[0] for r in rows]


def encode_rows(text_encoder, rows, device):
    """`rows` ([1, L] id tensors or id lists of one length) through the text encoder -> [R, L, C]: one native forward for a CLIP text model
    the route covers, else one call per row exactly as before (_encode_row_list)."""
    return torch.cat(_encode_row_list(text_encoder, rows, device), dim=0)


def encode_region_prompts(text_encoder, tokenizer, device, color_map_rgb, region_prompts, guidance_scale, like, dtype=None,
                          region_base_weight=0.0, region_feather=0.0):
    """One request's region prompts -> its plan for the sampler:
      "contexts"  K dicts built like the reference's unconditional dict (:355-357): the region prompt's embedding and the integer 0 in every
                  weight slot of `like` (the request's unconditional dict) -- plain cross-attention. Encoded to the chunk count of `like`.
      "masks"     fp32 [K, h, w] (ops.region_masks): the share of each latent pixel's 8 x 8 pixel block that has the region's colour,
                  feathered by `region_feather`
      "weights"   fp32 [K]: weight_k (1 - region_base_weight), formed in fp32
      "scales"    fp32 [K]: the region's guidance scale, the call's where it is None."""
    entries = region_entries(region_prompts)
    if color_map_rgb is None:
        raise ValueError("region_prompts need a color map")
    L = tokenizer.model_max_length
    k = like["CONTEXT_TENSOR"].shape[1] // L
    contexts = []
    # the K prompts' rows (k each) through the text encoder in one call: K k tensors [1, L, C]
    rows = []
    for _, prompt, _, _ in entries:
        if k <= 1:
            rows.append(tokenizer([prompt], padding="max_length", max_length=L, truncation=True, return_tensors="pt").input_ids)
        else:
            rows.extend(chunk_prompt(tokenizer, prompt, k, k)[1])
    embs = _encode_row_list(text_encoder, rows, device)
    kk = max(k, 1)
    for j in range(len(entries)):
        emb = embs[j] if k <= 1 else torch.cat(embs[j * kk:(j + 1) * kk], dim=1)
        if dtype is not None:
            emb = emb.to(dtype)
        ctx = {"CONTEXT_TENSOR": emb}
        ctx.update({key: 0 for key in dict.keys(like) if key.startswith("CROSS_ATTENTION_WEIGHT_")})
        contexts.append(ctx)
    rgb = torch.as_tensor(np.ascontiguousarray(color_map_rgb), dtype=torch.uint8).to(device)
    masks = ops.region_masks(rgb, [e[0] for e in entries], float(region_feather))
    keep = np.float32(1.0) - np.float32(region_base_weight)
    weights = torch.from_numpy(np.array([keep * np.float32(e[2]) for e in entries], dtype=np.float32))
    scales = torch.tensor([float(guidance_scale) if e[3] is None else e[3] for e in entries], dtype=torch.float32)
    return {"contexts": contexts, "masks": masks, "weights": weights.to(device), "scales": scales.to(device)}


def _parse_regions(color_context, tokenizer):
    """Host half of _image_context_seperator (:218-230): [(token_ids, (r, g, b), strength)]."""
    table = []
    for color, v in color_context.items():
        fields = v.split(",")
        strength = float(fields[-1])
        text = ",".join(fields[:-1])
        ids = tokenizer(text, max_length=tokenizer.model_max_length, truncation=True)["input_ids"][1:-1]
        if isinstance(color, str):
            color = (int(color[1:3], 16), int(color[3:5], 16), int(color[5:7], 16))
        table.append((list(ids), tuple(int(c) for c in color), strength))
    return table


MAX_PROMPT_CHUNKS = 3     # chunked prompt encoding: 77, 154 or 231 keys (libpww_hip_long.so serves 128 < M <= 256)


def check_prompt_chunks(max_prompt_chunks):
    """The `max_prompt_chunks` keyword of the entry points: an int in 1 .. MAX_PROMPT_CHUNKS."""
    if isinstance(max_prompt_chunks, bool) or not isinstance(max_prompt_chunks, int) or not 1 <= max_prompt_chunks <= MAX_PROMPT_CHUNKS:
        raise ValueError("max_prompt_chunks must be 1, 2 or %d (got %r): prompts of more than %d chunks are not supported"
                         % (MAX_PROMPT_CHUNKS, max_prompt_chunks, MAX_PROMPT_CHUNKS))
    return max_prompt_chunks


def _content_ids(tokenizer, text):
    """Token ids of `text` without truncation and without the BOS / EOS frame."""
    return list(tokenizer(text, max_length=1 << 20, truncation=False)["input_ids"][1:-1])


def prompt_chunk_count(tokenizer, prompt, max_prompt_chunks=1):
    """Chunks of model_max_length - 2 content tokens `prompt` needs, at most `max_prompt_chunks` (an empty prompt needs one)."""
    per = tokenizer.model_max_length - 2
    return max(1, min(check_prompt_chunks(max_prompt_chunks), -(-len(_content_ids(tokenizer, prompt)) // per)))


def chunk_prompt(tokenizer, prompt, max_prompt_chunks=1, min_chunks=1):
    """Chunked prompt encoding, host half: -> (content ids, id rows [k][model_max_length]). The content ids (no BOS / EOS) are split into
    chunks of model_max_length - 2; each chunk is framed BOS ... EOS and padded with EOS. k = the chunks the prompt needs, at least
    `min_chunks` (a batch pads every image to its largest k with empty chunks), at most `max_prompt_chunks`: content past the cap is cut."""
    L = tokenizer.model_max_length
    per = L - 2
    cap = check_prompt_chunks(max_prompt_chunks)
    ids = _content_ids(tokenizer, prompt)
    k = min(cap, max(1, min_chunks, -(-len(ids) // per)))
    ids = ids[:k * per]
    bos, eos = tokenizer("", max_length=L, truncation=True)["input_ids"][:2]
    rows = []
    for j in range(k):
        piece = ids[j * per:(j + 1) * per]
        rows.append([bos] + piece + [eos] * (L - 1 - len(piece)))
    return ids, rows


def framed_column(p, per=75):
    """Column of content position `p` in the concatenated chunks: every chunk adds a BOS in front and an EOS behind its `per` tokens."""
    return 1 + p + 2 * (p // per)


def framed_column_lists(table, content_ids, n_chunks, per=75):
    """_column_lists over the UNFRAMED content ids, scattered into the 77 k columns of the chunked prompt: a phrase that straddles a chunk
    boundary keeps all its columns, and nothing depends on where the split falls."""
    inner = _column_lists(table, content_ids)
    cols = [[] for _ in range(n_chunks * (per + 2))]
    for p, lst in enumerate(inner):
        cols[framed_column(p, per)] = lst
    return cols


def _column_lists(table, token_lis, ratio_tag="8"):
    """For every prompt position the region ordinals accumulated into it, in the reference's order
    (:257-268); warns like :270-271 when a phrase does not occur in the prompt."""
    cols = [[] for _ in token_lis]
    for r, (ids, _, _) in enumerate(table):
        L = len(ids)
        found = False
        for idx in range(len(token_lis)):
            if token_lis[idx: idx + L] == ids:
                found = True
                for c in range(idx, min(idx + L, len(token_lis))):
                    cols[c].append(r)
        if not found:
            print(f"Warning ratio {ratio_tag} : tokens {ids} not found in text")
    return cols


def gaussian_blur_mask(mask, sigma, ksize=39):
    """_blur_image_mask (:307-312): torchvision GaussianBlur(39x39, sigma) semantics on the device mask
    (pww_gauss_blur: two 1-D passes, reflect padding, fp64 accumulation)."""
    return ops.gauss_blur(mask, sigma, ksize)


def build_weight_maps(color_map_rgb, table, token_lis, device, extra_sigmas=None, with_orig=False, cols=None):
    """RGB map -> {N_8: [N, T], ...} fp32 device tensors, keyed like :370-377 -- ONE launch for the four resolutions -- plus
    "ORIG_THUNK": a callable that builds the [H, W, T] ratio-1 map on demand (with_orig=True: built now, key "ORIG").
    color_map_rgb: uint8 numpy / tensor [H, W, 3]. cols: the column lists, if the caller matched the phrases itself (chunked prompts:
    framed_column_lists); default: _column_lists over token_lis."""
    rgb = torch.as_tensor(np.ascontiguousarray(color_map_rgb), dtype=torch.uint8).to(device)
    H, W = rgb.shape[:2]
    if cols is None:
        cols = _column_lists(table, token_lis)
    regions = [(c[0], c[1], c[2], s) for (_, c, s) in table]
    ratios = (8, 16, 32, 64)
    blurred = {}
    if extra_sigmas:
        # blurred regions need float masks (:338-340): build them on device, blur (pww_gauss_blur), then accumulate
        print("Use extra sigma to smooth mask", extra_sigmas)
        masks = []
        for r, (_, c, s) in enumerate(table):
            m = (rgb == torch.tensor(c, dtype=torch.uint8, device=device)).all(dim=-1).float() * s
            if r in extra_sigmas:
                m = blurred[r] = gaussian_blur_mask(m, extra_sigmas[r])
            masks.append(m)
        masks = torch.stack(masks)
        outs = ops.mask_build_f32(masks, cols, ratios)
        orig_thunk = lambda: ops.mask_build_f32(masks, cols, (1,))[1].reshape(H, W, len(token_lis))      # noqa: E731
    else:
        outs = ops.mask_build(rgb, regions, cols, ratios)
        orig_thunk = lambda: ops.mask_build(rgb, regions, cols, (1,))[1].reshape(H, W, len(token_lis))    # noqa: E731
    maps = {}
    for r in ratios:
        maps[always_round(H / r) * always_round(W / r)] = outs[r]
    maps["ORIG_THUNK"] = orig_thunk
    if with_orig:
        maps["ORIG"] = orig_thunk()
    maps["_BLURRED"] = blurred      # region ordinal -> blurred float mask (region seeding thresholds these, :300-304)
    maps["_COLS"] = [c for c, lst in enumerate(cols) if lst]     # prompt positions that carry any region weight (:257-268)
    return maps


def _zero_weight_maps(keys, height, width, n_tokens, device):
    """The maps of an empty region table (:242-243): all-zero [N, T] per resolution and a thunk for the full-resolution one."""
    maps = {n: torch.zeros((n, n_tokens), dtype=torch.float32, device=device) for n in keys}
    maps["ORIG_THUNK"] = lambda: torch.zeros((height, width, n_tokens), dtype=torch.float32, device=device)
    return maps


def _warn_missing_colors(color_map_rgb, table):
    """:233-234."""
    img = np.asarray(color_map_rgb)
    for _, color, _ in table:
        if not (img == np.array(color, dtype=img.dtype)).all(axis=-1).any():
            print(f"Warning : not a single color {color} not found in image")


def _encode_text_color_inputs(text_encoder, tokenizer, device, color_map_image, color_context, input_prompt,
                              unconditional_input_prompt, dtype=None, use_sigma=True, max_prompt_chunks=1, min_prompt_chunks=1,
                              negative_color_context=None, negative_maps=False):
    """:315-388 with the weight maps built by the HIP mask kernel. Returns
    (extra_seeds, seperated_word_contexts, encoder_hidden_states, uncond_encoder_hidden_states);
    `seperated_word_contexts` is (region table [(token_ids, (r,g,b), strength)], rgb, {ordinal: blurred mask}) (the
    reference returns full-resolution float masks here; the only consumer, region seeding :451, gets what it
    needs from the table + color map, plus the blurred masks of the regions that carry a sigma).
    max_prompt_chunks > 1: a prompt of more than model_max_length - 2 tokens is encoded in up to that many chunks (chunk_prompt), each by
    the text encoder on its own, concatenated along the token axis: CONTEXT_TENSOR [1, 77 k, ctx], weight maps [N, 77 k]. A prompt that needs
    one chunk takes the code path of the default, whatever the cap. min_prompt_chunks: pad to that many chunks (per-image prompts of a batch).
    The chunk count is the larger of what the prompt and the unconditional prompt need under the cap.
    negative_color_context (extension; the grammar of color_context, read against the same color map, phrases matched in
    `unconditional_input_prompt`): the unconditional dict then carries weight maps of its own -- a PwWContext with
    CROSS_ATTENTION_WEIGHT_<N> tensors, a CROSS_ATTENTION_WEIGHT_ORIG built on first access and its own column bound -- which is exactly the
    dict the reference's builder returns as `cond` when it is called with (negative_color_context, unconditional_input_prompt). None or {}
    leave the unconditional dict as the reference builds it (the integer 0 in every weight slot). negative_maps=True: all-zero tensors
    instead of the integers when the context is empty (a batch in which only some requests carry one)."""
    chunk_rows = None
    if check_prompt_chunks(max_prompt_chunks) > 1:
        min_prompt_chunks = max(min_prompt_chunks, prompt_chunk_count(tokenizer, unconditional_input_prompt, max_prompt_chunks))
    if max_prompt_chunks > 1 or min_prompt_chunks > 1:
        content_ids, rows = chunk_prompt(tokenizer, input_prompt, max_prompt_chunks, min_prompt_chunks)
        if len(rows) > 1:
            chunk_rows = rows
    text_input = tokenizer([input_prompt], padding="max_length", max_length=tokenizer.model_max_length,
                           truncation=True, return_tensors="pt")
    color_context, extra_seeds, extra_sigmas = _extract_seed_and_sigma_from_context(color_context)
    neg_sigmas = {}
    if negative_color_context:
        check_negative_context(negative_color_context)
        if negative_color_context is not color_context:      # (one dict given for both sides: its tails are gone already)
            negative_color_context, _, neg_sigmas = _extract_seed_and_sigma_from_context(negative_color_context)
        else:
            neg_sigmas = dict(extra_sigmas)
    if not use_sigma:      # the pipeline classes parse the sigma tail and drop it (reference :574): no blur there
        extra_sigmas, neg_sigmas = {}, {}
    if color_map_image is None:
        # the reference's _image_context_seperator(None, ...) (:239-243): one dummy region over a 512 x 512 all-zero map --
        # plain Stable Diffusion (the pipeline class's default call, `pipe(prompt)`)
        rgb, height, width, table = None, 512, 512, []
    else:
        rgb = np.array(color_map_image.convert("RGB")) if hasattr(color_map_image, "convert") else np.asarray(color_map_image)
        height, width = rgb.shape[:2]
        table = _parse_regions(color_context, tokenizer)
    neg_table = _parse_regions(negative_color_context, tokenizer) if (negative_color_context and rgb is not None) else []
    token_lis = text_input["input_ids"][0].tolist() if chunk_rows is None else [t for row in chunk_rows for t in row]
    from . import attnmaps
    if attnmaps.active() is not None:       # (pww_hip.record_attention_maps: phrase lookup in the recorded maps needs the prompt's tokens)
        attnmaps.active().note_prompt(tokenizer, token_lis, None if chunk_rows is None else content_ids)
    keys = [always_round(height / r) * always_round(width / r) for r in (8, 16, 32, 64)]
    if table:
        _warn_missing_colors(rgb, table)
        cols = None if chunk_rows is None else framed_column_lists(table, content_ids, len(chunk_rows), tokenizer.model_max_length - 2)
        maps = build_weight_maps(rgb, table, token_lis, device, extra_sigmas, cols=cols)
        blurred = maps.pop("_BLURRED")
        nz_cols = maps.pop("_COLS")
    else:   # empty color_context (:242-243): all-zero maps
        maps = _zero_weight_maps(keys, height, width, len(token_lis), device)
        blurred = {}
        nz_cols = None

    if chunk_rows is None:
        uncond_input = tokenizer([unconditional_input_prompt], padding="max_length",
                                 max_length=text_input.input_ids.shape[-1], return_tensors="pt")
        cond_embeddings, uncond_embeddings = _encode_row_list(text_encoder, [text_input.input_ids, uncond_input.input_ids], device)      # one call
        uncond_lis, uncond_content = uncond_input["input_ids"][0].tolist(), None
    else:
        # every chunk through the text encoder on its own (it sees 77 positions, as it was trained), the unconditional prompt to the same k
        k = len(chunk_rows)
        uncond_content, uncond_rows = chunk_prompt(tokenizer, unconditional_input_prompt, k, k)
        uncond_lis = [t for row in uncond_rows for t in row]
        both = _encode_row_list(text_encoder, list(chunk_rows) + list(uncond_rows), device)            # 2 k rows: one call
        cond_embeddings, uncond_embeddings = torch.cat(both[:k], dim=1), torch.cat(both[k:], dim=1)
    if dtype is not None:
        cond_embeddings, uncond_embeddings = cond_embeddings.to(dtype), uncond_embeddings.to(dtype)

    # CROSS_ATTENTION_WEIGHT_ORIG (:343-345, :372) is built when somebody indexes it (PwWContext): only inj_forward's KeyError path does
    encoder_hidden_states = PwWContext({"CONTEXT_TENSOR": cond_embeddings}).set_lazy("CROSS_ATTENTION_WEIGHT_ORIG", maps["ORIG_THUNK"])
    if neg_table or (negative_maps and rgb is not None):
        # negative regions: one more build_weight_maps per request, over the unconditional prompt's tokens
        if neg_table:
            _warn_missing_colors(rgb, neg_table)
            ncols = None if chunk_rows is None else framed_column_lists(neg_table, uncond_content, len(chunk_rows), tokenizer.model_max_length - 2)
            nmaps = build_weight_maps(rgb, neg_table, uncond_lis, device, neg_sigmas, cols=ncols)
            nmaps.pop("_BLURRED")
            neg_nz = nmaps.pop("_COLS")
        else:
            nmaps = _zero_weight_maps(keys, height, width, len(uncond_lis), device)
            neg_nz = []
        uncond_encoder_hidden_states = PwWContext({"CONTEXT_TENSOR": uncond_embeddings}).set_lazy("CROSS_ATTENTION_WEIGHT_ORIG", nmaps["ORIG_THUNK"])
        for k in keys:
            uncond_encoder_hidden_states[f"CROSS_ATTENTION_WEIGHT_{k}"] = nmaps[k]
        from .attention import BIAS_COLS
        uncond_encoder_hidden_states[BIAS_COLS] = ((max(neg_nz) + 16) // 16 * 16) if neg_nz else 16
    else:
        uncond_encoder_hidden_states = {"CONTEXT_TENSOR": uncond_embeddings, "CROSS_ATTENTION_WEIGHT_ORIG": 0}
        for k in keys:
            uncond_encoder_hidden_states[f"CROSS_ATTENTION_WEIGHT_{k}"] = 0
    for k in keys:
        encoder_hidden_states[f"CROSS_ATTENTION_WEIGHT_{k}"] = maps[k]
    if nz_cols is not None:
        # Private, optional hints for the fused kernel (SURVEY.md 8b "may add private keys, must not require them"): only the
        # prompt positions covered by a region phrase are non-zero in ANY of the maps (5 - 17 of 77 for the shipped examples) --
        # the column bound, and the compact [N, R] + col_idx form of every per-resolution map.
        from .attention import BIAS_COLS, COMPACT_W, COMPACT_IDX
        # (both are kernel-launch geometry, i.e. part of a captured hipGraph's identity: rounded up -- the bound to 16 columns,
        # the compact width to 8 slots with unused ones marked -1 -- so that similar prompts replay the same graph)
        encoder_hidden_states[BIAS_COLS] = ((max(nz_cols) + 16) // 16 * 16) if nz_cols else 16
        # The compact form is OPT-IN (PWW_COMPACT_BIAS=1 / conditioning.COMPACT_BIAS): measured on MI355X it is 0.5 - 6 us SLOWER per
        # launch than the dense LDS tile bounded by BIAS_COLS in every UNet shape (profiles/r03_cross_timeline.md: the launch is bound
        # by the statistic hand-off and the score passes, not by the bias bytes), and building it costs 5 extra kernels per request.
        if COMPACT_BIAS and 1 <= len(nz_cols) <= ops.COMPACT_MAX_R:
            R = (len(nz_cols) + 7) // 8 * 8
            idx = torch.tensor(nz_cols, dtype=torch.int64, device=device)
            pad = torch.full((R - len(nz_cols),), -1, dtype=torch.int32, device=device)
            encoder_hidden_states[COMPACT_IDX] = torch.cat([idx.to(torch.int32), pad])
            for k in keys:
                wc = maps[k].new_zeros((maps[k].shape[0], R))
                wc[:, :len(nz_cols)] = maps[k].index_select(1, idx)
                encoder_hidden_states[COMPACT_W + str(k)] = wc
    return extra_seeds, (table, rgb, blurred), encoder_hidden_states, uncond_encoder_hidden_states


def _get_binary_mask(region_info, extra_seeds, dtype, size):
    """:300-304: per seeded region, (mask > 0) bilinearly resized (align_corners=False) to `size`. The reference
    thresholds the masks AFTER _blur_image_mask has replaced the blurred ones in place (:338-340), so a region given
    as "text,strength,seed,sigma" seeds the dilated area its blur reaches."""
    table, rgb = region_info[0], region_info[1]
    blurred = region_info[2] if len(region_info) > 2 else {}
    img = torch.as_tensor(rgb)
    out = []
    for k in extra_seeds.keys():
        _, color, strength = table[k]
        if k in blurred:
            m = (blurred[k].cpu() > 0).to(dtype)
        else:
            m = ((img == torch.tensor(color, dtype=img.dtype)).all(dim=-1).float() * strength > 0).to(dtype)
        out.append(F.interpolate(m[None, None], size=size, mode="bilinear"))
    return out
