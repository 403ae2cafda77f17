"""Drop-in for the reference module paint_with_words/paint_with_words.py (function API).

Same public names, signatures, defaults and context protocol as the reference (file:line cited per
function) so its runner.py works unchanged (`device="cuda:0"` is the HIP device under PyTorch-ROCm);
the attention arithmetic and the mask preparation run in hand-written gfx950 kernels
(libpww_hip.so, through pww_hip). This file is host glue: it owns no arithmetic of the hot path.

Beyond the reference's one-image-per-call API there is `paint_with_words_batch`: many
requests -- each with its own color map, color_context, prompt and seed -- through ONE denoise loop, CFG-folded and
hipGraph-replayed; image i of the batch equals the single-image call on request i (the reference generates several
samples by a sequential loop over seeds that reloads the model each time, gradio_pww.py:24-45).
"""
import math
import os
from functools import partial
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from PIL import Image

import pww_hip
from pww_hip.attention import inj_forward  # noqa: F401  (same import path as the reference's symbol)
from pww_hip.conditioning import check_prompt_chunks, prompt_chunk_count, check_negative_context
from pww_hip.conditioning import check_region_prompts, check_loras, region_entries, encode_region_prompts, check_region_strength
from pww_hip.conditioning import (always_round, _extract_seed_and_sigma_from_context, _encode_text_color_inputs,  # noqa: F401
                                  _get_binary_mask, gaussian_blur_mask)
from pww_hip.sampler import PwWSampler, initial_latents, canvas_plan, hold_first

try:  # the reference's dependency; absent in the offline build image
    from diffusers import AutoencoderKL, LMSDiscreteScheduler, UNet2DConditionModel
    _HAVE_DIFFUSERS = True
except Exception:  # pragma: no cover - depends on the environment
    from sd_standin import LMSDiscreteScheduler
    _HAVE_DIFFUSERS = False

# Execution mode of the denoise loop (see pww_hip/sampler.py): "eager" reproduces the reference's two
# batch-1 UNet calls per step; "folded"/"graph" batch cond+uncond (and replay hipGraphs).
DEFAULT_MODE = os.environ.get("PWW_MODE", "graph")


def preprocess_uint8(image):
    """What `preprocess` is made of: the image resized (LANCZOS) to the next lower multiple of 32, as the [1, H, W, 3] array of its pixels
    (uint8 for an RGB image)."""
    width, height = (side - side % 32 for side in image.size)
    return np.array(image.resize((width, height), resample=Image.LANCZOS))[None]


def preprocess(image):
    """reference :28-35: PIL image -> [-1, 1] NCHW tensor at the next lower multiple of 32."""
    pixels = preprocess_uint8(image).astype(np.float32) / 255.0
    return 2.0 * torch.from_numpy(pixels.transpose(0, 3, 1, 2)) - 1.0


def _encode_scaled(vae, image, device=None):
    """0.18215 * vae.encode(image).latent_dist.sample(): the scaled latent of an init image (:461, inpaint :213-226). image: a PIL image (it is
    preprocessed here and sent to `device`) or the tensor `vae.encode` is given.
    A VAE with the AutoencoderKL encoder layout in float16 / bfloat16 on a HIP device (pww_hip.vae_encode.covers) encodes on the native path,
    the noise drawn as `latent_dist.sample()` draws it; a PIL image goes there as its uint8 pixels (a quarter of the upload, no float image on
    the host) -> the fp32 latent. PWW_VAE_ENCODE=0, or any other VAE: the stock line, unchanged -> the latent in the VAE's dtype."""
    from pww_hip import vae_encode
    if vae_encode.enabled() and vae_encode.covers(vae):
        if isinstance(image, Image.Image):
            pixels = preprocess_uint8(image)
            if pixels.dtype == np.uint8 and pixels.ndim == 4 and pixels.shape[3] == 3:
                return vae_encode.encode(vae, torch.from_numpy(pixels).to(device=device), noise="sample")
            image = preprocess(image).to(device=device)
        return vae_encode.encode(vae, image.to(vae.dtype), noise="sample")
    if isinstance(image, Image.Image):
        image = preprocess(image).to(device=device)
    return 0.18215 * vae.encode(image.to(vae.dtype)).latent_dist.sample()


def _pil_from_latents(vae, latents, output_type="pil"):
    """reference :48-57: decode the latents, one PIL image per batch row -- or, for the pipeline classes' other output types, the
    [n, H, W, 3] float array of the diffusers pipeline's decode_latents (:821-833).
    A VAE with the AutoencoderKL decoder layout in float16 / bfloat16 on a HIP device (pww_hip.vae.covers) decodes on the native path: for
    PIL output the 8-bit image comes off the device as it is (one uint8 copy, no float image on the host), for the float output types the
    `.sample` form goes through the lines below. PWW_VAE=0, or any other VAE: the code below, unchanged."""
    from pww_hip import vae as native_vae
    if native_vae.enabled() and native_vae.covers(vae):
        z = (latents.clone() / 0.18215).to(vae.dtype)
        if output_type == "pil":
            return [Image.fromarray(im) for im in native_vae.decode(vae, z, "uint8").cpu().numpy()]
        decoded = native_vae.decode(vae, z, "sample")
    else:
        decoded = vae.decode((latents.clone() / 0.18215).to(vae.dtype)).sample
    pixels = (decoded / 2 + 0.5).clamp(0, 1).detach().float().cpu().permute(0, 2, 3, 1).numpy()
    if output_type != "pil":
        return pixels
    return [Image.fromarray(im) for im in (pixels * 255).round().astype("uint8")]


def pww_load_tools(device: str = "cuda:0", scheduler_type=LMSDiscreteScheduler, local_model_path: Optional[str] = None,
                   hf_model_path: Optional[str] = None, model_token: Optional[str] = None):
    """reference :128-204: load vae / unet / text encoder / tokenizer / scheduler and install the
    attention plug (:193-195). Needs diffusers + transformers and a model on disk or the hub; in an
    environment without them build the modules yourself and pass `preloaded_utils`."""
    assert local_model_path or hf_model_path, "either local_model_path or hf_model_path must be provided"
    if not _HAVE_DIFFUSERS:
        raise ImportError("pww_load_tools needs `diffusers` (the reference pins diffusers==0.10.0); it is not "
                          "installed here. Pass preloaded_utils=(vae, unet, text_encoder, tokenizer, scheduler).")
    from transformers import CLIPTextModel, CLIPTokenizer
    # the reference's two loading branches (:145-188): half weights from the checkpoint's `fp16` revision everywhere but on Apple's `mps`
    # device, where it loads fp32 from the default revision (kept for signature / behaviour parity: this package's kernels need a HIP device)
    half = device != "mps"
    model_path = local_model_path if local_model_path is not None else hf_model_path
    common = dict(use_auth_token=model_token, torch_dtype=torch.float16 if half else torch.float32, local_files_only=local_model_path is not None)
    if half:
        common["revision"] = "fp16"
    print(model_path)
    vae = AutoencoderKL.from_pretrained(model_path, subfolder="vae", **common)
    tokenizer = CLIPTokenizer.from_pretrained(model_path, subfolder="tokenizer")
    text_encoder = CLIPTextModel.from_pretrained(model_path, subfolder="text_encoder")
    unet = UNet2DConditionModel.from_pretrained(model_path, subfolder="unet", **common)
    vae.to(device), unet.to(device), text_encoder.to(device)
    if pww_hip.install(unet) == 0 and hasattr(unet, "set_attn_processor"):   # diffusers >= 0.12
        unet.set_attn_processor(pww_hip.PwWAttnProcessor())
    scheduler = scheduler_type(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                               num_train_timesteps=1000)
    return vae, unet, text_encoder, tokenizer, scheduler


def _tools(preloaded_utils, device, scheduler_type, local_model_path, hf_model_path, model_token):
    """(vae, unet, text_encoder, tokenizer, scheduler): the caller's `preloaded_utils`, or loaded as the reference does."""
    if preloaded_utils is not None:
        return preloaded_utils
    return pww_load_tools(device, scheduler_type, local_model_path=local_model_path, hf_model_path=hf_model_path, model_token=model_token)


def _unet_dtype(unet):
    return unet.dtype if hasattr(unet, "dtype") else next(unet.parameters()).dtype


def _sampler_for(unet, scheduler):
    """One PwWSampler (and its captured graphs) per (unet, scheduler, mode), kept on the unet. The mode is DEFAULT_MODE as it is NOW: every
    face of the package finds its sampler here, so assigning this module's global takes effect everywhere."""
    cache = unet.__dict__.setdefault("_pww_samplers", {})
    key = (id(scheduler), DEFAULT_MODE)
    if key not in cache:
        cache[key] = PwWSampler(unet, scheduler, DEFAULT_MODE)
    return cache[key]


# `sampler=` of the four function faces: name -> (class of sd_standin.schedulers, constructor keywords beside the betas and prediction_type)
SAMPLERS = {
    "euler": ("EulerDiscreteScheduler", {}),
    "euler_karras": ("EulerDiscreteScheduler", {"use_karras_sigmas": True}),
    "euler_a": ("EulerAncestralDiscreteScheduler", {}),
    "ddim": ("DDIMScheduler", {}),
    "dpmpp_2m": ("DPMSolverMultistepScheduler", {}),
    "dpmpp_2m_karras": ("DPMSolverMultistepScheduler", {"use_karras_sigmas": True}),
}


def check_sampler(sampler):
    """The `sampler` keyword, before any model is touched: None, or one of SAMPLERS' names (ValueError otherwise)."""
    if sampler is not None and (not isinstance(sampler, str) or sampler not in SAMPLERS):
        raise ValueError("sampler must be None or one of %s (got %r)" % (", ".join(sorted(SAMPLERS)), sampler))
    return sampler


def _named_scheduler(name, base):
    """The scheduler a `sampler=` name stands for, with the betas and the prediction_type of `base` (the scheduler in the tools)."""
    from sd_standin import schedulers
    config = getattr(base, "config", None) or {}
    get = config.get if hasattr(config, "get") else (lambda key, default=None: getattr(config, key, default))
    cls, kw = SAMPLERS[name]
    return getattr(schedulers, cls)(num_train_timesteps=get("num_train_timesteps", 1000), beta_start=get("beta_start", 0.00085),
                                    beta_end=get("beta_end", 0.012), beta_schedule=get("beta_schedule", "scaled_linear"),
                                    prediction_type=get("prediction_type", None) or "epsilon", **kw)


def _broadcast(value, n, name):
    """A per-request argument of paint_with_words_batch: one value for every request, or a sequence of n."""
    if isinstance(value, (list, tuple)) and not (name == "color_context" and isinstance(value, dict)):
        if len(value) != n:
            raise ValueError("%s has %d entries for %d requests" % (name, len(value), n))
        return list(value), False
    return [value] * n, True


def _batch_prompt_chunks(tokenizer, prompts, max_prompt_chunks):
    """Chunks every image of a call is encoded to: the largest count any of its prompts needs under the cap (1 with the default cap)."""
    if check_prompt_chunks(max_prompt_chunks) == 1:
        return 1
    return max(prompt_chunk_count(tokenizer, p, max_prompt_chunks) for p in prompts)


def _negative_contexts(negative_color_contexts, n, color_map_images):
    """-> ([one negative_color_context or None per request], does any request carry one). A request without a color map has no regions
    on either side."""
    negs = list(negative_color_contexts) if negative_color_contexts is not None else [None] * n
    negs = [c if (c and color_map_images[i] is not None) else None for i, c in enumerate(negs)]
    return negs, any(c is not None for c in negs)


def _region_requests(region_prompts, n):
    """-> one `region_prompts` dict per request, or None when no request carries one (None and {} are "off")."""
    regs = list(region_prompts) if isinstance(region_prompts, (list, tuple)) else [region_prompts] * n
    return regs if any(regs) else None


def _batch_requests(n, color_contexts, negative_color_context, color_map_images, input_prompts, strip_color_contexts):
    """The per-request arguments a batch function shares with its twin -> (color contexts, negative contexts, color maps, prompts: n of
    each; `shared`: every request has the same four, so one conditioning serves all; the caller's dicts to strip after the call). Not
    shared: one dict may serve several requests, so a private copy per request is parsed and the caller's dicts -- the negative ones, and
    the color contexts if `strip_color_contexts` -- lose their tails afterwards, each object once."""
    ctxs, s1 = _broadcast(color_contexts, n, "color_context")
    negs, s4 = _broadcast(negative_color_context, n, "negative_color_context")
    maps, s2 = _broadcast(color_map_images, n, "color_map_images")
    prompts, s3 = _broadcast(input_prompts, n, "input_prompts")
    if s1 and s2 and s3 and s4:
        return ctxs, negs, maps, prompts, True, []
    strip = {id(c): c for c in (ctxs if strip_color_contexts else []) + [c for c in negs if c]}
    return [dict(c) for c in ctxs], [dict(c) if c else None for c in negs], maps, prompts, False, list(strip.values())


CANVAS_MAX_WINDOW, CANVAS_MAX_WINDOWS, CANVAS_MAX_RAMP = 1024, 64, 64     # pixels; windows per canvas and ramp length (include/pww_hip_canvas.h)


def _canvas_request(size, canvas_window, canvas_stride, canvas_ramp):
    """The `canvas_window` / `canvas_stride` / `canvas_ramp` keywords of paint_with_words against the color map's (width, height) -> None
    (the plain call: no window, or a canvas no larger than the window on both axes) or the sampler's canvas_plan in latent pixels."""
    if canvas_window is None:
        return None
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)      # noqa: E731
    if not is_int(canvas_window) or canvas_window % 64 or not 64 <= canvas_window <= CANVAS_MAX_WINDOW:
        raise ValueError("canvas_window must be a multiple of 64 pixels in 64 .. %d (got %r)" % (CANVAS_MAX_WINDOW, canvas_window))
    stride = canvas_window // 2 if canvas_stride is None else canvas_stride
    if not is_int(stride) or stride % 8 or not 8 <= stride <= canvas_window:
        raise ValueError("canvas_stride must be a multiple of 8 pixels in 8 .. canvas_window = %d (got %r)" % (canvas_window, canvas_stride))
    if not is_int(canvas_ramp) or not 0 <= canvas_ramp <= CANVAS_MAX_RAMP:
        raise ValueError("canvas_ramp must be an integer number of latent pixels in 0 .. %d (got %r)" % (CANVAS_MAX_RAMP, canvas_ramp))
    width, height = size
    if width <= canvas_window and height <= canvas_window:
        return None
    if width % 8 or height % 8:
        raise ValueError("canvas: the sides of a canvas larger than the window must be multiples of 8 pixels (the color map is %d x %d)" % (width, height))
    if width < canvas_window or height < canvas_window:
        raise ValueError("canvas: the %d x %d color map is smaller than the window of %d pixels on one axis" % (width, height, canvas_window))
    plan = canvas_plan((height // 8, width // 8), canvas_window // 8, stride // 8, canvas_ramp)
    if len(plan["ys"]) * len(plan["xs"]) > CANVAS_MAX_WINDOWS:
        raise ValueError("canvas: %d x %d windows of %d pixels every %d pixels cover the %d x %d color map: more than %d (use a larger stride or window)"
                         % (len(plan["ys"]), len(plan["xs"]), canvas_window, stride, width, height, CANVAS_MAX_WINDOWS))
    return plan


def _canvas_conditioning(encode, canvas, color_map, color_context, negative_color_context):
    """The conditioning of a canvas request: every window is an image of its own whose color map is the crop of the canvas map under it.
    encode(color map, color_context, negative_color_context) is _generate's call of _encode_text_color_inputs.
    -> (conds, unconds, region tables: one per window in window order; the (extra_seeds, region_info) of the CANVAS for the initial latent).
    The dicts are parsed once per window, so every window but the last parses a private copy with the seed / sigma tails still on; the last
    parses the caller's own dicts, which lose their tails once, as in the plain call. Region seeds are read against the canvas map: a
    context that carries one is parsed once more at canvas size for the initial latent (without one nothing is built at canvas size)."""
    h, w = canvas["window"]
    boxes = [(8 * x0, 8 * y0, 8 * (x0 + w), 8 * (y0 + h)) for y0 in canvas["ys"] for x0 in canvas["xs"]]
    seeds_info = ({}, None)
    if _extract_seed_and_sigma_from_context(dict(color_context))[1]:
        extra_seeds, region_info, _, _ = encode(color_map, dict(color_context), None)
        seeds_info = (extra_seeds, region_info)
    conds, unconds, tables = [], [], []
    for i, box in enumerate(boxes):
        last = i == len(boxes) - 1
        ctx = color_context if last else dict(color_context)
        neg = negative_color_context if last or not negative_color_context else dict(negative_color_context)
        _, region_info, cond, uncond = encode(color_map.crop(box), ctx, neg)
        conds.append(cond), unconds.append(uncond), tables.append(region_info)
    return conds, unconds, tables, seeds_info


def _seeded_noise(tools, device, seeds, timesteps, seeds_info, sizes):
    """txt2img (:444-457): CPU-generated latents per seed exactly as :446, with the region seeds; `sizes`: (width, height) per request."""
    unet, scheduler = tools[1], tools[4]
    lats = [initial_latents(seed, unet.in_channels, height, width, extra_seeds=extra_seeds,
                            region_masks=lambda dtype, size, ri=region_info, es=extra_seeds: _get_binary_mask(ri, es, dtype, size))
            for seed, (width, height), (extra_seeds, region_info) in zip(seeds, sizes, seeds_info)]
    return torch.cat(lats, dim=0).to(device) * scheduler.init_noise_sigma, None


def _held_images(tools, device, seeds, timesteps, seeds_info, init_images, made_of=True):
    """img2img (:459-468): the init images through the VAE encoder, noised to the first timestep (noise from the global generator) -- and what
    they were made of: -> (latents, None, the encoded init latents x0, the noise z), the last two for a request with region strengths
    (made_of=False: not formed)."""
    vae, scheduler = tools[0], tools[4]
    lats, inits, noises = [], [], []
    for init_image in init_images:
        init_latents = _encode_scaled(vae, init_image, device).float()
        noise = torch.randn(init_latents.shape).to(device)
        lats.append(scheduler.add_noise(init_latents, noise, timesteps[:1]))
        inits.append(init_latents), noises.append(noise)
    if not made_of:
        return torch.cat(lats, dim=0), None
    return torch.cat(lats, dim=0), None, torch.cat(inits, dim=0), torch.cat(noises, dim=0)


def _noised_images(tools, device, seeds, timesteps, seeds_info, init_images):
    """img2img (:459-468): the init images through the VAE encoder, noised to the first timestep (noise from the global generator)."""
    return _held_images(tools, device, seeds, timesteps, seeds_info, init_images, made_of=False)


def _hold_request(entries, feather, strength, num_inference_steps, color_map_images, init_images):
    """The region strengths of a call (check_region_strength's entries, one list or None per request; None: the feature is off -> None)
    against what else the call was given, before any model is touched -> the `hold` argument of _generate: {"entries", "feather", "base":
    `strength`, the strength of every pixel whose colour is not named, "steps": T, "first": i0, the first step of the T-step schedule the
    request runs: the step that releases the largest strength any request names (sampler.hold_first), whether or not the colour occurs in
    a map}. ValueError: a base strength outside [0, 1], a call whose largest strength releases nothing in T steps, a color map that is not
    8 x the latent the init image encodes to (its size at the next lower multiple of 32)."""
    if entries is None:
        return None
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 <= float(strength) <= 1.0:      # (a NaN fails the comparison)
        raise ValueError("region_strength: `strength`, the strength of every pixel whose colour is not named, must be a number in [0, 1] (got %r)" % (strength,))
    if isinstance(num_inference_steps, bool) or not isinstance(num_inference_steps, int) or num_inference_steps < 1:
        raise ValueError("region_strength: num_inference_steps must be a positive integer (got %r)" % (num_inference_steps,))
    for color_map, init_image in zip(color_map_images, init_images):
        if color_map is None:
            raise ValueError("region_strength needs a color map")
        latent = tuple(side - side % 32 for side in init_image.size)
        if tuple(color_map.size) != latent:
            raise ValueError("region_strength: the color map is %d x %d but the init image encodes to a latent of %d x %d pixels / 8: the color map must "
                             "be 8 x the latent on both axes" % (tuple(color_map.size) + latent))
    top = max([float(strength)] + [s for e in entries if e is not None for _, s in e])
    first = hold_first(num_inference_steps, top)
    if first >= num_inference_steps:
        raise ValueError("region_strength: the largest strength of the call (%g) releases no pixel in %d steps: nothing would be denoised"
                         % (top, num_inference_steps))
    return {"entries": entries, "feather": float(feather), "base": float(strength), "steps": num_inference_steps, "first": first}


def _hold_scheduler_check(scheduler):
    """Region strengths count the steps of the schedule from its start and noise the init latent per step: a scheduler that shifts its
    timesteps (`steps_offset`) or cannot add noise is refused, before the conditioning is formed."""
    config = getattr(scheduler, "config", None)
    offset = (config.get("steps_offset", 0) if hasattr(config, "get") else getattr(config, "steps_offset", 0)) or 0
    if offset != 0:
        raise ValueError("region_strength: a scheduler with steps_offset = %r is not supported (%s)" % (offset, type(scheduler).__name__))
    if not hasattr(scheduler, "add_noise"):
        raise ValueError("region_strength needs a scheduler with add_noise (%s has none)" % type(scheduler).__name__)


def _strength_maps(hold, color_map_images, device):
    """S, fp32 [n, h, w]: the strength map of every request from its color map (ops.hold_strength_map: one launch, two more with a feather);
    a request that names no colour has the base strength everywhere. Requests that share a map and a dict share the launches."""
    made, out = {}, []
    for color_map, entries in zip(color_map_images, hold["entries"]):
        key = (id(color_map), id(entries))
        if key not in made:
            if entries is None:
                width, height = color_map.size
                made[key] = torch.full((height // 8, width // 8), float(np.float32(hold["base"])), dtype=torch.float32, device=device)
            else:
                rgb = torch.as_tensor(np.ascontiguousarray(np.array(color_map.convert("RGB"))), dtype=torch.uint8).to(device)
                made[key] = pww_hip.ops.hold_strength_map(rgb, [e[0] for e in entries], [e[1] for e in entries], hold["base"], hold["feather"])
        out.append(made[key])
    return torch.stack(out, dim=0)


CONTROL_MAX_NETS = 4      # ControlNets per call (pww_hip.controlnet.MAX_NETS)


def _control_image_tensor(image, size):
    """One control image -> float32 [3, H, W] in [0, 1]: a PIL image, a uint8 array [H, W, 3] (or [H, W]), or a float tensor [3, H, W] (or
    [1, 3, H, W]) in [0, 1]. It must have the size of the color map, (width, height) = `size`."""
    width, height = size
    if torch.is_tensor(image):
        t = image[0] if image.dim() == 4 and image.shape[0] == 1 else image
        if t.dim() != 3 or t.shape[0] != 3 or not t.is_floating_point():
            raise ValueError("control_image: a tensor must be a float [3, H, W] in [0, 1] (got %s %s)" % (tuple(image.shape), image.dtype))
        if tuple(t.shape[1:]) != (height, width):
            raise ValueError("control_image is %d x %d but the color map is %d x %d: they must have the same size" % (t.shape[2], t.shape[1], width, height))
        t = t.detach().float().cpu()
        if t.numel() and not (float(t.min()) >= 0.0 and float(t.max()) <= 1.0):
            raise ValueError("control_image: a tensor must lie in [0, 1] (got %g .. %g)" % (float(t.min()), float(t.max())))
        return t
    if isinstance(image, Image.Image):
        arr = np.array(image.convert("RGB"))
    elif isinstance(image, np.ndarray):
        arr = image
    else:
        raise ValueError("control_image must be a PIL image, a uint8 array or a float tensor in [0, 1] (got %s)" % type(image).__name__)
    if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] != 3):
        raise ValueError("control_image: an array must be uint8 [H, W, 3] or [H, W] (got %s %s)" % (arr.shape, arr.dtype))
    if arr.ndim == 2:
        arr = np.repeat(arr[:, :, None], 3, axis=2)
    if arr.shape[:2] != (height, width):
        raise ValueError("control_image is %d x %d but the color map is %d x %d: they must have the same size" % (arr.shape[1], arr.shape[0], width, height))
    return torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).float() / 255.0


def _control_request(controlnet, control_image, scale, start, end, n, size):
    """The `controlnet` / `control_image` / `controlnet_conditioning_scale` / `control_guidance_start` / `control_guidance_end` keywords of a
    call of n images whose color maps are `size` -> None (no ControlNet) or the sampler's pww_hip.controlnet.ControlRequest. One net takes one
    image (for every image of the call) or a list of n; a list of nets takes a list with such an entry per net."""
    if controlnet is None:
        if control_image is not None:
            raise ValueError("control_image without a controlnet")
        return None
    many = isinstance(controlnet, (list, tuple))
    nets = list(controlnet) if many else [controlnet]
    if not 1 <= len(nets) <= CONTROL_MAX_NETS:
        raise ValueError("controlnet: %d nets (1 .. %d)" % (len(nets), CONTROL_MAX_NETS))
    if control_image is None:
        raise ValueError("controlnet needs a control_image")
    if many and (not isinstance(control_image, (list, tuple)) or len(control_image) != len(nets)):
        raise ValueError("controlnet: a list of %d nets takes a list of %d control images" % (len(nets), len(nets)))
    images = []
    for entry in (control_image if many else [control_image]):
        rows = list(entry) if isinstance(entry, (list, tuple)) else [entry] * n
        if len(rows) != n:
            raise ValueError("control_image has %d entries for %d requests" % (len(rows), n))
        made = {}
        for r in rows:
            if id(r) not in made:
                made[id(r)] = _control_image_tensor(r, size)
        images.append(torch.stack([made[id(r)] for r in rows], dim=0))
    scales = list(scale) if isinstance(scale, (list, tuple)) else [scale] * len(nets)
    if len(scales) != len(nets) or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in scales):
        raise ValueError("controlnet_conditioning_scale must be a number or one per net (got %r for %d nets)" % (scale, len(nets)))
    for v in (start, end):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError("control_guidance_start / control_guidance_end must be numbers in [0, 1] (got %r, %r)" % (start, end))
    return pww_hip.controlnet.ControlRequest(nets, images, scales, start, end)


def _txt2img_or_img2img(sizes, init_images, strength):
    """-> the (`start`, `strength`) arguments of _generate for a face that takes optional init images."""
    if init_images is None:
        return partial(_seeded_noise, sizes=sizes), None
    return partial(_noised_images, init_images=init_images), strength


def _generate(tools, device, color_contexts, color_map_images, prompts, seeds, num_inference_steps, guidance_scale, weight_function,
              unconditional_input_prompt, start, strength=None, map_sizes=None, on_step=None, use_region_sigma=True, shared=False,
              max_prompt_chunks=1, negative_color_contexts=None, negative_strength=1.0, region_prompts=None, region_base_weight=0.0,
              region_feather=0.0, loras=None, canvas=None, hold=None, control=None, sampler_name=None):
    """The body behind every face of the package (reference :414-506, paint_with_words_inpaint.py:160-262): conditioning per request (once
    if `shared`: every request has the same map, context and prompt), the timesteps, the initial state, one denoise loop over all images.
    Returns the final latents [n, 4, h, w].
    start(tools, device, seeds, timesteps, seeds_info) -> (latents [n, 4, h, w], extra UNet input channels [n, 5, h, w] or None) is the
    initial state: _seeded_noise, _noised_images or the inpaint module's _inpaint_start. strength: None runs every timestep (txt2img), a
    number the img2img tail of the schedule (:434-441). map_sizes: one (width, height) per request to resize its color map to (the inpaint
    function API, paint_with_words_inpaint.py:172). negative_color_contexts: None, or one dict (or None) per request like color_contexts --
    regions of the unconditional prompt (see paint_with_words). region_prompts: None, or one dict per request (_region_requests) -- a full
    prompt per colour, blended per latent pixel where guidance is combined (see paint_with_words). loras: None, or what check_loras made of the
    `lora` / `region_loras` keywords. canvas: None, or the plan of ONE request whose color map is larger than the UNet's window
    (_canvas_request): the conditioning is formed per window on the crop of the map, the initial state at canvas size. hold: None, or the
    region strengths of an img2img call (_hold_request): `start` is then _held_images, the request runs the schedule from hold["first"], and
    the sampler is handed the init latents, the noise and one strength map per request (at canvas size for a canvas request). control: None,
    or the ControlNets of the call (_control_request), handed to the sampler as they are. sampler_name: None, or the `sampler` keyword of
    the call (check_sampler): the request runs on that scheduler, built for this call from the tools' scheduler's config, on the tools'
    PwWSampler -- so a captured graph serves every scheduler."""
    unet, text_encoder, tokenizer, scheduler = tools[1:]
    n = len(seeds)
    base = scheduler
    if sampler_name is not None:
        scheduler = _named_scheduler(sampler_name, base)
        tools = tuple(tools[:4]) + (scheduler,)
    if hold is not None:
        _hold_scheduler_check(scheduler)
    sampler = _sampler_for(unet, base)   # also installs the attention plug
    conds, unconds, seeds_info = [], [], []
    region_texts = [e[1] for r in (region_prompts or []) for e in region_entries(r)]
    min_chunks = _batch_prompt_chunks(tokenizer, (prompts[:1] if shared else prompts) + [unconditional_input_prompt] + region_texts, max_prompt_chunks)
    negs, any_neg = _negative_contexts(negative_color_contexts, n, color_map_images)
    if canvas is not None:
        encode = lambda color_map, ctx, neg: _encode_text_color_inputs(      # noqa: E731
            text_encoder, tokenizer, device, color_map, ctx, prompts[0], unconditional_input_prompt, dtype=_unet_dtype(unet), use_sigma=use_region_sigma,
            max_prompt_chunks=max_prompt_chunks, min_prompt_chunks=min_chunks, negative_color_context=neg, negative_maps=any_neg)
        conds, unconds, tables, canvas_seeds = _canvas_conditioning(encode, canvas, color_map_images[0], color_contexts[0], negs[0])
        n_w, shared = len(conds), False
        seeds_info = [canvas_seeds]
    for i in range(0 if canvas is not None else 1 if shared else n):
        color_map = color_map_images[i]
        if map_sizes is not None and color_map is not None:
            color_map = color_map.resize(map_sizes[i], Image.NEAREST)
        extra_seeds, region_info, cond, uncond = _encode_text_color_inputs(
            text_encoder, tokenizer, device, color_map, color_contexts[i], prompts[i], unconditional_input_prompt,
            dtype=_unet_dtype(unet), use_sigma=use_region_sigma, max_prompt_chunks=max_prompt_chunks, min_prompt_chunks=min_chunks,
            negative_color_context=negs[i], negative_maps=any_neg)
        conds.append(cond), unconds.append(uncond), seeds_info.append((extra_seeds, region_info))
    regions = None
    if region_prompts and canvas is not None:
        # one plan per window: the region masks (and their feather) are formed on the window's crop of the color map
        regions = [encode_region_prompts(text_encoder, tokenizer, device, table[1], region_prompts[0], guidance_scale, uncond, dtype=_unet_dtype(unet),
                                         region_base_weight=region_base_weight, region_feather=region_feather) for table, uncond in zip(tables, unconds)]
    elif region_prompts:
        # one plan per request (one for all when the requests share everything): K more rows of the same UNet evaluation
        one = shared and all(r is region_prompts[0] for r in region_prompts)
        regions = [encode_region_prompts(text_encoder, tokenizer, device, seeds_info[0 if shared else i][1][1], region_prompts[i], guidance_scale,
                                         unconds[0 if shared else i], dtype=_unet_dtype(unet), region_base_weight=region_base_weight,
                                         region_feather=region_feather) for i in range(1 if one else n)]
    if shared:
        conds, unconds, seeds_info = conds[0], unconds[0], seeds_info * n

    scheduler.set_timesteps(num_inference_steps)
    timesteps = scheduler.timesteps
    if hold is not None:
        timesteps = timesteps[hold["first"]:]
    elif strength is not None:
        offset = scheduler.config.get("steps_offset", 0)
        init_timestep = min(int(num_inference_steps * strength) + offset, num_inference_steps)
        timesteps = timesteps[max(num_inference_steps - init_timestep + offset, 0):]

    latents, extra_channels, *made_of = start(tools, device, seeds, timesteps, seeds_info)
    more = {} if regions is None else {"regions": regions}        # (a call without region prompts is, argument for argument, the call of before)
    if hold is not None:
        # (the VAE's convolution may hand its output back in channels_last memory: the hold launch reads NCHW)
        more["hold"] = {"init": made_of[0].contiguous(), "noise": made_of[1].contiguous(), "strength": _strength_maps(hold, color_map_images, device), "steps": hold["steps"],
                        "first": hold["first"]}
    if canvas is not None:
        more["canvas"] = canvas
    if control is not None:
        more["control"] = control
    if loras is not None:
        rows = n if canvas is None else n_w         # (the rows of a canvas request are its windows: the one request's adapters for each of them)
        colors = [[e[0] for e in region_entries(r)] for r in region_prompts] if region_prompts else [[]] * n
        region_loras = loras[1] if canvas is None or loras[1] is None else list(loras[1]) * n_w
        more["lora_rows"] = pww_hip.lora.row_plan(rows, colors if canvas is None else colors * n_w, loras[0], region_loras, pww_hip.lora.state_of(unet).index)
    with pww_hip.miopen_find():
        if scheduler is base:
            return sampler.sample(conds, unconds, latents, timesteps, guidance_scale, weight_function, extra_channels=extra_channels,
                                  on_step=on_step, negative_strength=negative_strength, **more)
        sampler.scheduler = scheduler      # for this call only
        try:
            return sampler.sample(conds, unconds, latents, timesteps, guidance_scale, weight_function, extra_channels=extra_channels,
                                  on_step=on_step, negative_strength=negative_strength, **more)
        finally:
            sampler.scheduler = base


def _finish(tools, latents, return_latents=False, decode=None):
    """What a face returns for the final latents: the latents themselves (`return_latents`), or the decoded images -- a list of PIL images,
    or what the pipeline classes' `decode` makes of _pil_from_latents. Either way a fused hand-off that timed out raises here instead of
    handing back NaNs."""
    sampler = _sampler_for(tools[1], tools[4])
    if return_latents:
        return sampler.checked(latents)
    images = (decode or _pil_from_latents)(tools[0], latents)
    sampler.check_errors()     # (the decode above synchronised already)
    return images


@torch.no_grad()
def paint_with_words(
    color_context: Dict[Tuple[int, int, int], str] = {},
    color_map_image: Optional[Image.Image] = None,
    input_prompt: str = "",
    num_inference_steps: int = 30,
    guidance_scale: float = 7.5,
    seed: int = 0,
    scheduler_type=LMSDiscreteScheduler,
    device: str = "cuda:0",
    weight_function: Callable = lambda w, sigma, qk: 0.1 * w * math.log(sigma + 1) * qk.max(),
    local_model_path: Optional[str] = None,
    hf_model_path: Optional[str] = "CompVis/stable-diffusion-v1-4",
    preloaded_utils: Optional[Tuple] = None,
    unconditional_input_prompt: str = "",
    model_token: Optional[str] = None,
    init_image: Optional[Image.Image] = None,
    strength: float = 0.5,
    return_latents: bool = False,
    negative_color_context: Optional[Dict[Tuple[int, int, int], str]] = None,
    negative_strength: float = 1.0,
    region_strength=None,
    region_strength_feather: float = 0.0,
    lora=None,
    region_loras=None,
    canvas_window: Optional[int] = None,
    canvas_stride: Optional[int] = None,
    canvas_ramp: int = 0,
    controlnet=None,
    control_image=None,
    controlnet_conditioning_scale=1.0,
    control_guidance_start: float = 0.0,
    control_guidance_end: float = 1.0,
    sampler: Optional[str] = None,
    region_prompts=None,
    region_base_weight: float = 0.0,
    region_feather: float = 0.0,
    max_prompt_chunks: int = 1,
):
    """reference :391-510. `return_latents=True` (extension) returns the final latent tensor instead
    of decoding it -- the quantity parity is checked on. `negative_color_context` (extension; the reference's README lists "negative
    region" as an open item): regions of the UNCONDITIONAL prompt, in the grammar of color_context ("phrase,strength[,-1[,sigma]]", a region
    seed is refused) and read against the same color map; the phrases are looked up in `unconditional_input_prompt`. The unconditional
    evaluation of every step then adds `negative_strength * weight_function(w_neg, sigma, qk_uncond)` to its cross-attention scores, so
    classifier-free guidance pushes away from the phrase inside its region. None / {} (the default) is the reference's unconditional pass.
    The dict is stripped of its seed / sigma tails like color_context. `max_prompt_chunks` (extension; 1, 2 or 3): a prompt longer than 75 tokens is
    encoded in up to that many 75-token chunks (154 / 231 keys) instead of cut at 77; with the default every request is tokenized as in
    the reference, and a prompt that needs fewer chunks than the cap gets only the chunks it needs.
    `region_prompts` (extension; the reference's README lists "sentence wise text separation" as open): a full prompt per colour of the
    color map, {(r, g, b): "prompt"} or {(r, g, b): ("prompt", weight in (0, 1], guidance_scale or None)}, 1 to 8 regions; the colours need
    not appear in color_context. Every region prompt is one more row of each UNet evaluation (plain cross-attention, no token weights), and
    the noise predictions are blended per latent pixel where guidance is combined: with M_k the share of the pixel's 8 x 8 block that has
    colour k (feathered by a Gaussian of `region_feather` latent pixels, at most 8) and w_k = (1 - region_base_weight) weight_k M_k,
    noise = e_u + (1 - sum w_k) g (e_prompt - e_u) + sum_k w_k s_k (e_k - e_u) -- `input_prompt` keeps the share `region_base_weight`
    in [0, 1) inside the regions and everything outside them; s_k is region k's guidance scale (the call's by default). None / {} is the
    call without the feature. Not combined with negative_color_context.
    `lora` / `region_loras` (extension): LoRA adapters loaded with pww_hip.lora.load_lora(unet, source, name) on the UNet of
    `preloaded_utils`, applied unmerged and per row of the UNet evaluation: lora = "name" or ("name", scale) is the adapter of the prompt's
    row, the unconditional row and every region without an adapter of its own (alone it behaves like merged weights); region_loras =
    {(r, g, b) | "#rrggbb": "name" | ("name", scale)} gives a colour of region_prompts its own adapter.
    `canvas_window` / `canvas_stride` / `canvas_ramp` (extension): a color map larger than `canvas_window` pixels (a multiple of 64, at most
    1024; square windows) is denoised as overlapping windows of that size, one every `canvas_stride` pixels (a multiple of 8 in 8 ..
    canvas_window; None: half the window) with the last window of an axis clamped to the canvas's end, at most 64 windows (MultiDiffusion,
    Bar-Tal et al. 2023): per step the windows are the images of ONE UNet evaluation and the mean of their noise predictions per latent pixel
    -- weighted, with canvas_ramp > 0 (latent pixels, at most 64), by a linear ramp min(distance to the window's edge + 1, canvas_ramp) along
    each axis -- takes one scheduler step on the canvas. A window is an image of its own for conditioning: its color map is the crop of the
    canvas map under it, and blur sigmas, negative regions, region masks and their feather are formed on the crop; a colour that is absent
    from a window gives zero maps there. The score statistic a weight_function reads (qk.max() ...) is per window, because it is per image.
    The initial latent (with region seeds, against the whole map) and the img2img encoding are formed at canvas size. None (the default), or
    a map no larger than the window on both axes, is the plain call; a map smaller than the window on one axis, a side that is not a
    multiple of 8, more than 64 windows or a value out of range raise ValueError. record_attention_maps() is refused around such a call.
    Not part of this: the *_batch forms, the inpaint function, both pipeline classes, windows spread over several GPUs, non-square windows.
    `region_strength` / `region_strength_feather` (extension, img2img only; Differential Diffusion, Levin and Fried 2023): a denoising
    strength per colour of the color map, {(r, g, b) | "#rrggbb": s} with s in [0, 1], 1 to 8 colours that need not appear in color_context
    -- "repaint the lake hard, touch the sky lightly, leave the house alone" on a stock 4-channel UNet. `strength` stays the strength of
    every pixel whose colour is not named. Per latent pixel S = strength + sum_k M_k (s_k - strength), M_k the share of the pixel's 8 x 8
    block that has colour k, clamped to [0, 1] and feathered by a Gaussian of `region_strength_feather` latent pixels (at most 8). With T =
    num_inference_steps a pixel is released at step g iff S >= (T - g) / T (in fp32; equality releases); the call runs the schedule from the
    step that releases the largest strength it names -- whether or not that colour occurs in the map, so the step count does not depend on
    the picture -- and after every scheduler step one launch puts the pixels the next step does not release back to the init latent noised to
    that step's timestep (with the request's one noise tensor). Pixels that are never released come back as the encoded init latent, bit
    for bit; if every named strength equals `strength` the result is the plain img2img call's. It composes with negative regions, region
    prompts, LoRA adapters, long prompts and canvases (the strength map is then formed at canvas size). None / {} is the call without the
    feature. ValueError: no init_image, a strength outside [0, 1], more than 8 colours, a colour named twice, a feather outside [0, 8], a
    color map that is not 8 x the latent, strengths that release nothing in T steps, a scheduler with steps_offset or without add_noise.
    `controlnet` / `control_image` / `controlnet_conditioning_scale` / `control_guidance_start` / `control_guidance_end` (extension; the
    reference's README chapter "Paint with Words + ControlNet"): a ControlNet -- or a list of at most 4 -- beside the color map: the control
    image (scribble, depth, segmentation ...) steers the geometry, the color map which word goes where. control_image: a PIL image, a uint8
    array or a float tensor in [0, 1] of the color map's size (a list of nets takes a list of images); the scale: a number or one per net;
    the ControlNets act on the steps i of T with control_guidance_start <= i / T and (i + 1) / T <= control_guidance_end. A net must have the
    layout pww_hip.controlnet.covers takes, in float16 / bfloat16 on the UNet's device. txt2img and img2img, every mode; it composes with
    negative regions, region prompts, LoRA adapters (which act on the UNet alone), long prompts and region strength. Scale 0, or an empty
    window, is the call without a ControlNet. ValueError: an image of another size, together with canvas_window. Not part of this: the
    inpaint functions (a 9-channel UNet has no 4-channel ControlNet), the pipeline classes, pww_hip.dist.
    `sampler` (extension; the reference's README lists "Support for other schedulers"): None (the default) samples with the scheduler in the
    tools -- `preloaded_utils[4]`, or what `scheduler_type` loaded: the call of before. A name -- "euler", "euler_karras", "euler_a", "ddim",
    "dpmpp_2m", "dpmpp_2m_karras" -- samples THIS call with that scheduler (sd_standin.schedulers: Euler, Euler ancestral, DDIM with eta 0,
    DPM-Solver++(2M); `_karras`: Karras sigmas, rho 7), built with the betas and the prediction_type of the scheduler in the tools, which is
    left as it is. These schedulers take every step as one native launch (pww_hip.steps; PWW_STEP=0: their own step()), and in hipGraph mode
    the graph captured for one serves all. They compose with negative regions, region prompts, LoRA adapters, long prompts, ControlNets,
    canvases, img2img and inpainting. region_strength with a name that builds a steps_offset = 1 scheduler ("ddim", "dpmpp_2m",
    "dpmpp_2m_karras") stays refused (ValueError): pass a scheduler constructed with steps_offset=0 in `preloaded_utils` (or a
    `scheduler_type` that builds one) instead -- that is accepted. Any other value: ValueError, before any model is touched. The pipeline
    classes take the scheduler they are constructed with."""
    check_sampler(sampler)
    check_prompt_chunks(max_prompt_chunks)
    check_negative_context(negative_color_context, negative_strength)
    check_region_prompts(region_prompts, region_base_weight, region_feather, negative_color_context)
    held = check_region_strength(region_strength, region_strength_feather, None if init_image is None else [init_image])
    loras = check_loras(lora, region_loras, region_prompts, tools=preloaded_utils)
    color_map_image.size     # the reference dereferences it unconditionally (:414): None raises here too
    canvas = _canvas_request(color_map_image.size, canvas_window, canvas_stride, canvas_ramp)
    if controlnet is not None and canvas_window is not None:
        raise ValueError("controlnet does not combine with canvas_window (the hint would have to be cropped per window)")
    control = _control_request(controlnet, control_image, controlnet_conditioning_scale, control_guidance_start, control_guidance_end, 1, color_map_image.size)
    hold = _hold_request(held, region_strength_feather, strength, num_inference_steps, [color_map_image], [init_image])
    tools = _tools(preloaded_utils, device, scheduler_type, local_model_path, hf_model_path, model_token)
    start, strength = _txt2img_or_img2img([color_map_image.size], None if init_image is None else [init_image], strength)
    more = {} if canvas is None else {"canvas": canvas}
    if hold is not None:      # (a call without region strengths is, argument for argument, the call of before)
        start, more["hold"] = partial(_held_images, init_images=[init_image]), hold
    if control is not None:   # (and so is a call without a ControlNet)
        more["control"] = control
    if sampler is not None:   # (and so is a call without a sampler name)
        more["sampler_name"] = sampler
    latents = _generate(tools, device, [color_context], [color_map_image], [input_prompt], [seed], num_inference_steps, guidance_scale,
                        weight_function, unconditional_input_prompt, start, strength, shared=True, max_prompt_chunks=max_prompt_chunks,
                        negative_color_contexts=[negative_color_context], negative_strength=negative_strength,
                        region_prompts=_region_requests(region_prompts, 1), region_base_weight=region_base_weight, region_feather=region_feather,
                        loras=loras, **more)
    out = _finish(tools, latents, return_latents)
    return out if return_latents else out[0]


@torch.no_grad()
def paint_with_words_batch(
    color_contexts: Union[Dict, Sequence[Dict]],
    color_map_images: Union[Image.Image, Sequence[Image.Image]],
    input_prompts: Union[str, Sequence[str]],
    seeds: Sequence[int],
    num_inference_steps: int = 30,
    guidance_scale: float = 7.5,
    scheduler_type=LMSDiscreteScheduler,
    device: str = "cuda:0",
    weight_function: Callable = lambda w, sigma, qk: 0.1 * w * math.log(sigma + 1) * qk.max(),
    local_model_path: Optional[str] = None,
    hf_model_path: Optional[str] = "CompVis/stable-diffusion-v1-4",
    preloaded_utils: Optional[Tuple] = None,
    unconditional_input_prompt: str = "",
    model_token: Optional[str] = None,
    init_images: Union[None, Image.Image, Sequence[Image.Image]] = None,
    strength: float = 0.5,
    return_latents: bool = False,
    negative_color_context: Union[None, Dict, Sequence[Optional[Dict]]] = None,
    negative_strength: float = 1.0,
    region_strength=None,
    region_strength_feather: float = 0.0,
    lora=None,
    region_loras=None,
    controlnet=None,
    control_image=None,
    controlnet_conditioning_scale=1.0,
    control_guidance_start: float = 0.0,
    control_guidance_end: float = 1.0,
    sampler: Optional[str] = None,
    region_prompts=None,
    region_base_weight: float = 0.0,
    region_feather: float = 0.0,
    max_prompt_chunks: int = 1,
):
    """len(seeds) requests through ONE denoise loop (the reference's multi-sample path is a
    sequential loop of paint_with_words calls, gradio_pww.py:24-45). `color_contexts`, `color_map_images`,
    `input_prompts` and `init_images` are either one value shared by every request or a sequence with one entry per
    seed; each image has its own weight maps (kernel argument bias_stride[0]), prompt embedding, per-image score
    statistic and region seeds, so image i equals `paint_with_words(color_contexts[i], color_map_images[i],
    input_prompts[i], seed=seeds[i], ...)`. All color maps of one call must have the same size. The caller's
    color_context dicts are mutated like the single-image call mutates its dict (:296). Returns a list of PIL images
    (or the [n, 4, h, w] latents with return_latents=True). negative_color_context / negative_strength: see paint_with_words; one dict
    shared by every request or one (or None) per seed, like color_contexts. max_prompt_chunks: see paint_with_words; with per-image prompts
    every image is padded (with empty chunks) to the largest chunk count of the batch. region_prompts / region_base_weight / region_feather:
    see paint_with_words; one dict for all requests or one per seed, every request with the same number of regions. lora / region_loras: see
    paint_with_words; `lora` serves every request, region_loras is one dict for all requests or one (or None) per seed. region_strength /
    region_strength_feather: see paint_with_words; one dict for all requests or one (or None) per seed -- all requests run the same steps:
    from the step that releases the largest strength any of them names. controlnet / control_image / controlnet_conditioning_scale /
    control_guidance_start / control_guidance_end: see paint_with_words; control_image is one image for all requests or one per seed (with a
    list of nets: a list with such an entry per net). sampler: see paint_with_words; one name for every request."""
    check_sampler(sampler)
    check_prompt_chunks(max_prompt_chunks)
    check_negative_context(negative_color_context, negative_strength)
    seeds = list(seeds)
    n = len(seeds)
    check_region_prompts(region_prompts, region_base_weight, region_feather, negative_color_context, n_requests=n)
    held = check_region_strength(region_strength, region_strength_feather, init_images, n_requests=n)
    loras = check_loras(lora, region_loras, region_prompts, n_requests=n, tools=preloaded_utils)
    if n == 0:
        return []
    ctxs, negs, maps, prompts, shared, strip = _batch_requests(n, color_contexts, negative_color_context, color_map_images, input_prompts,
                                                               strip_color_contexts=True)
    inits = None if init_images is None else _broadcast(init_images, n, "init_images")[0]
    if len({m.size for m in maps}) != 1:
        raise ValueError("paint_with_words_batch: all color maps of one call must have the same size, got %s"
                         % sorted({m.size for m in maps}))
    hold = _hold_request(held, region_strength_feather, strength, num_inference_steps, maps, inits or [])
    control = _control_request(controlnet, control_image, controlnet_conditioning_scale, control_guidance_start, control_guidance_end, n, maps[0].size)
    tools = _tools(preloaded_utils, device, scheduler_type, local_model_path, hf_model_path, model_token)
    start, strength = _txt2img_or_img2img([m.size for m in maps], inits, strength)
    more = {}
    if hold is not None:      # (a call without region strengths is, argument for argument, the call of before)
        start, more["hold"] = partial(_held_images, init_images=inits), hold
    if control is not None:   # (and so is a call without a ControlNet)
        more["control"] = control
    if sampler is not None:   # (and so is a call without a sampler name)
        more["sampler_name"] = sampler
    latents = _generate(tools, device, ctxs, maps, prompts, seeds, num_inference_steps, guidance_scale, weight_function,
                        unconditional_input_prompt, start, strength, shared=shared, max_prompt_chunks=max_prompt_chunks,
                        negative_color_contexts=negs, negative_strength=negative_strength, region_prompts=_region_requests(region_prompts, n),
                        region_base_weight=region_base_weight, region_feather=region_feather, loras=loras, **more)
    for c in strip:
        _extract_seed_and_sigma_from_context(c)
    return _finish(tools, latents, return_latents)


def __getattr__(name):
    """The reference defines its pipeline class in this module (:513); here it lives in pipelines.py (which imports this
    module), so the name resolves lazily."""
    if name == "PaintWithWord_StableDiffusionPipeline":
        from .pipelines import PaintWithWord_StableDiffusionPipeline
        return PaintWithWord_StableDiffusionPipeline
    raise AttributeError(name)
