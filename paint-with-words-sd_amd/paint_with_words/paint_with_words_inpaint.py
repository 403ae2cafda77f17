"""Drop-in for the reference module paint_with_words/paint_with_words_inpaint.py (function API):
the inpainting variant feeds a 9-channel UNet input cat([latents, mask, masked_image_latents])
(reference :237, :250); the attention path is the same fused HIP op, and the mask / masked-image
preparation (reference :20-134) is one HIP kernel (pww_inpaint_prep) over the uint8 pixels."""
import math
from functools import partial
from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from pww_hip import ops
from .paint_with_words import (LMSDiscreteScheduler, _tools, _generate, _finish, _broadcast, _batch_requests, check_prompt_chunks,
                               check_negative_context, check_region_prompts, check_loras, _region_requests, preprocess, _encode_scaled,
                               _extract_seed_and_sigma_from_context, check_sampler)


def _as_uint8_pixels(image, channels):
    """PIL image or numpy array -> uint8 numpy array ([H, W, 3] for channels == 3, [H, W] for 1), or None when the
    values are not 8-bit pixels (float arrays go through the tensor path)."""
    if isinstance(image, Image.Image):
        return np.asarray(image.convert("RGB" if channels == 3 else "L"))
    arr = np.asarray(image)
    return arr if arr.dtype == np.uint8 else None


def _prep_on_device(rgb_u8, mask_u8, device, lat_hw=None):
    """(mask [1,1,H,W], masked_image [1,3,H,W], latent-size mask or None) from uint8 pixels, on `device`."""
    H, W = mask_u8.shape
    h, w = lat_hw if lat_hw is not None else (max(H // 8, 1), max(W // 8, 1))
    m, masked, ml = ops.inpaint_prep(torch.from_numpy(np.ascontiguousarray(rgb_u8)).to(device),
                                     torch.from_numpy(np.ascontiguousarray(mask_u8)).to(device), h, w)
    return m, masked, ml


def prepare_mask_and_masked_image(image, mask, device=None):
    """reference :20-106: (image, mask) -> (mask [B,1,H,W] in {0,1}, masked_image [B,3,H,W] in [-1,1] with the masked
    pixels zeroed). 8-bit inputs (PIL images / uint8 arrays -- what the reference's callers pass, runner_inpaint.py:
    44-46) are converted by pww_inpaint_prep when `device` is a HIP device; tensors (the reference's second input form:
    image in [-1,1], mask in [0,1], optional batch / channel axes) are checked and thresholded where they live."""
    image_is_tensor, mask_is_tensor = torch.is_tensor(image), torch.is_tensor(mask)
    if image_is_tensor != mask_is_tensor:
        which, other, bad = ("image", "mask", mask) if image_is_tensor else ("mask", "image", image)
        raise TypeError(f"`{which}` is a torch.Tensor but `{other}` (type: {type(bad)} is not")
    if image_is_tensor:
        image = image[None] if image.ndim == 3 else image
        if mask.ndim == 2:
            mask = mask[None, None]
        elif mask.ndim == 3:       # [1, H, W] is one mask with its channel axis, [B, H, W] a batch without one
            mask = mask[None] if mask.shape[0] == 1 else mask[:, None]
        if image.ndim != 4 or mask.ndim != 4 or image.shape[1] != 3:
            raise AssertionError("Image must be (3, H, W) or (B, 3, H, W) and Mask (H, W), (1, H, W), (B, H, W) or (B, 1, H, W)")
        if image.shape[-2:] != mask.shape[-2:] or image.shape[0] != mask.shape[0]:
            raise AssertionError("Image and Mask must have the same spatial dimensions and batch size")
        if image.min() < -1 or image.max() > 1:
            raise ValueError("Image should be in [-1, 1] range")
        if mask.min() < 0 or mask.max() > 1:
            raise ValueError("Mask should be in [0, 1] range")
        mask = (mask >= 0.5).to(mask.dtype)
        image = image.to(torch.float32)
        return mask, image * (mask < 0.5)
    rgb, m8 = _as_uint8_pixels(image, 3), _as_uint8_pixels(mask, 1)
    if rgb is not None and m8 is not None and device is not None and torch.device(device).type == "cuda":
        m, masked, _ = _prep_on_device(rgb, m8, device)
        return m, masked
    # float arrays (already scaled masks) or no HIP device named: the same arithmetic as host tensors
    rgb = np.asarray(image.convert("RGB")) if isinstance(image, Image.Image) else np.asarray(image)
    pix = torch.from_numpy(np.ascontiguousarray(rgb)).permute(2, 0, 1)[None].to(torch.float32) / 127.5 - 1.0
    m = np.asarray(mask.convert("L")).astype(np.float32) / 255.0 if isinstance(mask, Image.Image) else np.asarray(mask, dtype=np.float32)
    m = torch.from_numpy((m >= 0.5).astype(np.float32))[None, None]
    return m, pix * (m < 0.5)


def prepare_mask_latents(vae, mask, masked_image, batch_size, height, width, dtype, device, generator,
                         do_classifier_free_guidance):
    """reference :109-134: mask to latent resolution (nearest), masked image through the VAE encoder, both repeated
    per batch row (and doubled for a CFG-concatenated batch)."""
    mask = F.interpolate(mask, size=(height // 8, width // 8)).to(device=device, dtype=dtype)
    latent = _encode_scaled(vae, masked_image.to(device=device, dtype=vae.dtype))
    reps = batch_size * (2 if do_classifier_free_guidance else 1)
    return mask.repeat(reps, 1, 1, 1), latent.repeat(reps, 1, 1, 1).to(device=device, dtype=dtype)


def _inpaint_inputs(vae, init_image, mask_image, seed, scheduler, timesteps, device, mask_hw=None):
    """One request's (noised latents [1,4,h,w], extra channels [1,5,h,w]) -- reference :201-228. `mask_hw`: the pipeline
    class sizes the latent mask by its `height` / `width` arguments (:498-508) instead of by the init image."""
    width, height = init_image.size
    if mask_hw is not None:
        height, width = mask_hw
    generator = torch.manual_seed(seed)
    image = preprocess(init_image).to(device=device)
    init_latents = _encode_scaled(vae, image).float()
    noise = torch.randn(init_latents.shape, generator=generator).to(device)
    latents = scheduler.add_noise(init_latents, noise, timesteps[:1])

    rgb, m8 = _as_uint8_pixels(init_image, 3), _as_uint8_pixels(mask_image, 1)
    _, masked_image, mask_lat = _prep_on_device(rgb, m8, device, lat_hw=(height // 8, width // 8))
    masked_latents = _encode_scaled(vae, masked_image).to(latents.dtype)
    if mask_hw is not None and (mask_lat.shape[-2:] != latents.shape[-2:] or masked_latents.shape[-2:] != latents.shape[-2:]):
        # the reference's pipeline fails in torch.cat here (:532): `height` / `width` must be the size of `image`
        raise ValueError(f"`height` x `width` = {height} x {width} gives a {tuple(mask_lat.shape[-2:])} latent mask but `image` gives "
                         f"{tuple(latents.shape[-2:])} latents: pass the size of `image` (a multiple of 32)")
    if mask_lat.shape[-2:] != latents.shape[-2:]:      # sizes that `preprocess` rounds down to a multiple of 32 (:213-214)
        mask_lat = F.interpolate(mask_lat, size=latents.shape[-2:], mode="nearest")
        masked_latents = F.interpolate(masked_latents, size=latents.shape[-2:], mode="nearest")
    return latents, torch.cat([mask_lat.to(latents.dtype), masked_latents], dim=1)


def _inpaint_start(tools, device, seeds, timesteps, seeds_info, init_images, mask_images, mask_hw=None, resize_inputs=True):
    """The initial state of an inpainting request for _generate: noised init-image latents plus cat([mask, masked-image latents]) for the
    9-channel UNet. The function API resizes the mask to the init image (:173, `resize_inputs`); the pipeline class does not and sizes the
    latent mask by `mask_hw`."""
    vae, unet, scheduler = tools[0], tools[1], tools[4]
    lats, extras = [], []
    for init_image, mask_image, seed in zip(init_images, mask_images, seeds):
        if resize_inputs:
            mask_image = mask_image.resize(init_image.size, Image.NEAREST)
        if mask_image.size != init_image.size:
            raise AssertionError("Image and Mask must have the same spatial dimensions")                            # :72-73
        lat, extra = _inpaint_inputs(vae, init_image, mask_image, seed, scheduler, timesteps, device, mask_hw=mask_hw)
        lats.append(lat), extras.append(extra)
    latents, extra = torch.cat(lats, dim=0), torch.cat(extras, dim=0)
    n_lat, n_extra = latents.shape[1], extra.shape[1]
    if n_lat + n_extra != unet.in_channels:
        config = getattr(unet, "config", None)
        raise ValueError(
            f"Incorrect configuration settings! The config of `pipeline.unet`: {config} expects {unet.in_channels} input "
            f"channels but received {n_lat} latent + 1 mask + {n_extra - 1} masked-image latent channels = {n_lat + n_extra}. "
            "Please verify the config of `pipeline.unet` or your `mask_image` or `image` input.")
    return latents, extra


def _no_controlnet(controlnet, control_image):
    """The inpaint functions carry the keywords only to answer them: their UNet reads 9 channels and a ControlNet reads the latent's 4."""
    if controlnet is not None or control_image is not None:
        raise ValueError("controlnet / control_image are not part of the inpaint functions: a 9-channel inpainting UNet has no 4-channel ControlNet "
                         "(use paint_with_words or paint_with_words_batch)")


@torch.no_grad()
def paint_with_words_inpaint(
    color_context: Dict[Tuple[int, int, int], str] = {},
    color_map_image: Optional[Image.Image] = None,
    mask_image: Optional[Image.Image] = None,
    init_image: Image.Image = None,
    input_prompt: str = "",
    num_inference_steps: int = 150,
    guidance_scale: float = 7.5,
    seed: int = 0,
    scheduler_type=LMSDiscreteScheduler,
    device: str = "cuda:0",
    weight_function: Callable = lambda w, sigma, qk: 0.1 * w * math.log(sigma + 1) * qk.max(),
    local_model_path: Optional[str] = None,
    hf_model_path: Optional[str] = "runwayml/stable-diffusion-inpainting",
    preloaded_utils: Optional[Tuple] = None,
    unconditional_input_prompt: str = "",
    model_token: Optional[str] = None,
    strength: float = 1.0,
    return_latents: bool = False,
    negative_color_context: Optional[Dict[Tuple[int, int, int], str]] = None,
    negative_strength: float = 1.0,
    lora=None,
    region_loras=None,
    controlnet=None,
    control_image=None,
    sampler: Optional[str] = None,
    region_prompts=None,
    region_base_weight: float = 0.0,
    region_feather: float = 0.0,
    max_prompt_chunks: int = 1,
):
    """reference :137-270. negative_color_context / negative_strength / region_prompts / region_base_weight / region_feather /
    max_prompt_chunks / lora / region_loras (extensions): see paint_with_words; controlnet / control_image are refused (ValueError). The region masks are read from the color map resized to the init image: its size
    must be 8 x the latent's (a multiple of 32). sampler (extension): see paint_with_words."""
    check_sampler(sampler)
    check_prompt_chunks(max_prompt_chunks)
    _no_controlnet(controlnet, control_image)
    check_negative_context(negative_color_context, negative_strength)
    check_region_prompts(region_prompts, region_base_weight, region_feather, negative_color_context)
    loras = check_loras(lora, region_loras, region_prompts, tools=preloaded_utils)
    tools = _tools(preloaded_utils, device, scheduler_type, local_model_path, hf_model_path, model_token)
    latents = _generate(tools, device, [color_context], [color_map_image], [input_prompt], [seed], num_inference_steps, guidance_scale,
                        weight_function, unconditional_input_prompt, partial(_inpaint_start, init_images=[init_image], mask_images=[mask_image]),
                        strength, map_sizes=[init_image.size], shared=True, max_prompt_chunks=max_prompt_chunks,
                        negative_color_contexts=[negative_color_context], negative_strength=negative_strength,
                        region_prompts=_region_requests(region_prompts, 1), region_base_weight=region_base_weight, region_feather=region_feather,
                        loras=loras, **({} if sampler is None else {"sampler_name": sampler}))
    out = _finish(tools, latents, return_latents)
    return out if return_latents else out[0]


@torch.no_grad()
def paint_with_words_inpaint_batch(
    color_contexts: Union[Dict, Sequence[Dict]],
    color_map_images: Union[Image.Image, Sequence[Image.Image]],
    mask_images: Union[Image.Image, Sequence[Image.Image]],
    init_images: Union[Image.Image, Sequence[Image.Image]],
    input_prompts: Union[str, Sequence[str]],
    seeds: Sequence[int],
    num_inference_steps: int = 150,
    guidance_scale: float = 7.5,
    scheduler_type=LMSDiscreteScheduler,
    device: str = "cuda:0",
    weight_function: Callable = lambda w, sigma, qk: 0.1 * w * math.log(sigma + 1) * qk.max(),
    local_model_path: Optional[str] = None,
    hf_model_path: Optional[str] = "runwayml/stable-diffusion-inpainting",
    preloaded_utils: Optional[Tuple] = None,
    unconditional_input_prompt: str = "",
    model_token: Optional[str] = None,
    strength: float = 1.0,
    return_latents: bool = False,
    negative_color_context: Union[None, Dict, Sequence[Optional[Dict]]] = None,
    negative_strength: float = 1.0,
    lora=None,
    region_loras=None,
    controlnet=None,
    control_image=None,
    sampler: Optional[str] = None,
    region_prompts=None,
    region_base_weight: float = 0.0,
    region_feather: float = 0.0,
    max_prompt_chunks: int = 1,
):
    """len(seeds) inpainting requests through one denoise loop (see paint_with_words_batch): each of the image-like
    arguments and the prompt is one shared value or a sequence with one entry per seed; all init images of a call must
    have the same size. Image i equals the single-request call on request i. negative_color_context / negative_strength /
    region_prompts / region_base_weight / region_feather / max_prompt_chunks / lora / region_loras / sampler: see paint_with_words_batch."""
    check_sampler(sampler)
    check_prompt_chunks(max_prompt_chunks)
    _no_controlnet(controlnet, control_image)
    check_negative_context(negative_color_context, negative_strength)
    seeds = list(seeds)
    n = len(seeds)
    check_region_prompts(region_prompts, region_base_weight, region_feather, negative_color_context, n_requests=n)
    loras = check_loras(lora, region_loras, region_prompts, n_requests=n, tools=preloaded_utils)
    if n == 0:
        return []
    # (private copies are parsed when the requests differ; this function strips the caller's negative dicts only afterwards)
    ctxs, negs, maps, prompts, shared, strip = _batch_requests(n, color_contexts, negative_color_context, color_map_images, input_prompts,
                                                               strip_color_contexts=False)
    masks, _ = _broadcast(mask_images, n, "mask_images")
    inits, _ = _broadcast(init_images, n, "init_images")
    if len({im.size for im in inits}) != 1:
        raise ValueError("paint_with_words_inpaint_batch: all init images of one call must have the same size")
    tools = _tools(preloaded_utils, device, scheduler_type, local_model_path, hf_model_path, model_token)
    latents = _generate(tools, device, ctxs, maps, prompts, seeds, num_inference_steps, guidance_scale, weight_function,
                        unconditional_input_prompt, partial(_inpaint_start, init_images=inits, mask_images=masks), strength,
                        map_sizes=[im.size for im in inits], shared=shared, max_prompt_chunks=max_prompt_chunks,
                        negative_color_contexts=negs, negative_strength=negative_strength, region_prompts=_region_requests(region_prompts, n),
                        region_base_weight=region_base_weight, region_feather=region_feather, loras=loras,
                        **({} if sampler is None else {"sampler_name": sampler}))
    for c in strip:
        _extract_seed_and_sigma_from_context(c)
    return _finish(tools, latents, return_latents)


def __getattr__(name):
    """reference paint_with_words_inpaint.py:273 defines the inpaint pipeline class in this module"""
    if name == "PaintWithWord_StableDiffusionInpaintPipeline":
        from .pipelines import PaintWithWord_StableDiffusionInpaintPipeline
        return PaintWithWord_StableDiffusionInpaintPipeline
    raise AttributeError(name)
