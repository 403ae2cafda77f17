"""Pipeline-class face of the same algorithm (reference paint_with_words.py:513-842 and
paint_with_words_inpaint.py:273-575). The reference subclasses diffusers' StableDiffusionPipeline (not installable
offline); these classes keep the reference's constructor / `from_pretrained` / `plugin_cross_attention` / `__call__`
signatures -- argument names, ORDER and defaults -- and run the shared generation body of the function API.

Behaviour the reference's pipeline variant has and the function API has not, kept on purpose:
  * height / width default to `unet.config.sample_size * 8` and size the LATENT; the color map only sizes the weight
    maps (:700-701, :756);
  * the per-region blur sigma is parsed and dropped (:574); `eta` doubles as the img2img strength (:735);
  * `latents`, `generator` and `num_images_per_prompt` are accepted and not used (:744-753 is commented out in the
    reference; the latents always come from `seed`): passing a non-default value warns once instead of failing;
  * the inpaint class takes color map and mask as given (no resize to the init image, unlike the function API :172-173),
    sizes the latent mask by `height` / `width` (paint_with_words_inpaint.py:427-432, :498-508 -- they must be the size of
    `image`) and calls `callback(i, t, latents)` every `callback_steps` steps (:555-559);
  * the safety checker never runs (`nsfw_content_detected` is False, :829).
"""
import math
import warnings
from functools import partial
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Tuple, Union

import torch
from PIL import Image

import pww_hip
from .paint_with_words import (LMSDiscreteScheduler, _generate, _finish, _pil_from_latents, _txt2img_or_img2img, check_prompt_chunks,
                               check_negative_context, check_region_prompts, check_loras, _region_requests, check_region_strength, _hold_request,
                               _held_images)
from .paint_with_words_inpaint import _inpaint_start

_warned = set()


def _unused(name, value, default):
    if value is not default and value != default and name not in _warned:
        _warned.add(name)
        warnings.warn("%s is accepted for signature compatibility and not used (the reference's pipeline ignores it too)" % name)


def _decode(vae, latents, output_type):
    """decode_latents + numpy_to_pil of the diffusers pipeline (:821-833), by the package's one decoder: [n, H, W, 3] float array or PIL images."""
    return _pil_from_latents(vae, latents, output_type)


class PaintWithWord_StableDiffusionPipeline:
    # extension: `pipe.max_prompt_chunks = 2` / `3` encodes a prompt of more than 75 tokens in that many 75-token chunks at the most (see
    # paint_with_words). An attribute, because the constructor and `__call__` keep exactly the reference's parameter lists.
    max_prompt_chunks = 1
    # extension: negative regions (see paint_with_words): `pipe.negative_color_context = {(r, g, b): "phrase,strength"}` -- phrases of
    # `negative_prompt`, read against the call's color map -- and `pipe.negative_strength`. Attributes for the same reason.
    negative_color_context = None
    negative_strength = 1.0
    # extension: region prompts (see paint_with_words): `pipe.region_prompts = {(r, g, b): "full prompt"}` -- a prompt per colour of the call's
    # color map, blended per latent pixel -- with `pipe.region_base_weight` and `pipe.region_feather`. Attributes for the same reason.
    region_prompts = None
    region_base_weight = 0.0
    region_feather = 0.0
    # extension: LoRA adapters (see paint_with_words), loaded with pww_hip.lora.load_lora(pipe.unet, source, name): `pipe.lora = "name"` or
    # `("name", scale)`, `pipe.region_loras = {(r, g, b): "name"}` for the colours of `pipe.region_prompts`. Attributes for the same reason.
    lora = None
    region_loras = None
    # extension: region strength (see paint_with_words), img2img only: `pipe.region_strength = {(r, g, b): s}` -- a denoising strength per
    # colour of the call's color map, `eta` being the strength of every other pixel -- and `pipe.region_strength_feather`. Attributes for the
    # same reason. The inpaint class does not take them.
    region_strength = None
    region_strength_feather = 0.0
    # ControlNets (see paint_with_words) are not part of the pipeline classes: setting `pipe.controlnet` is answered with a ValueError.
    controlnet = None

    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler=None, safety_checker=None, feature_extractor=None,
                 requires_safety_checker: bool = False):
        self.vae, self.text_encoder, self.tokenizer, self.unet = vae, text_encoder, tokenizer, unet
        self.safety_checker, self.feature_extractor = safety_checker, feature_extractor
        # the reference replaces whatever scheduler it is given by LMSDiscrete (:533-538)
        self.scheduler = LMSDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                              num_train_timesteps=1000)
        self.vae_scale_factor = 8
        self.device = next(unet.parameters()).device
        self.plugin_cross_attention()

    @classmethod
    def from_pretrained(cls, save_dir, **kwargs):
        """reference :541-554. `save_dir` is a local directory or a hub id; `torch_dtype`, `revision`, `use_auth_token`,
        `local_files_only` ... go to diffusers' loader untouched when diffusers is installed."""
        try:
            from diffusers import StableDiffusionPipeline
        except Exception as e:
            raise ImportError("from_pretrained needs `diffusers` (the reference pins diffusers==0.10.0); build the modules "
                              "yourself and call %s(vae, text_encoder, tokenizer, unet, ...)" % cls.__name__) from e
        sd = StableDiffusionPipeline.from_pretrained(save_dir, **kwargs)
        return cls(vae=sd.vae, text_encoder=sd.text_encoder, tokenizer=sd.tokenizer, unet=sd.unet, scheduler=sd.scheduler,
                   safety_checker=getattr(sd, "safety_checker", None), feature_extractor=getattr(sd, "feature_extractor", None),
                   requires_safety_checker=getattr(sd, "requires_safety_checker", False))

    def to(self, device):
        for m in (self.vae, self.text_encoder, self.unet):
            m.to(device)
        self.device = torch.device(device)
        return self

    def plugin_cross_attention(self):
        """reference :556-559"""
        if pww_hip.install(self.unet) == 0 and hasattr(self.unet, "set_attn_processor"):
            self.unet.set_attn_processor(pww_hip.PwWAttnProcessor())

    def _default_side(self):
        cfg = getattr(self.unet, "config", None)
        size = cfg.get("sample_size") if isinstance(cfg, dict) else getattr(cfg, "sample_size", None)
        return (size or 64) * self.vae_scale_factor

    def _check_extensions(self):
        if self.controlnet is not None:
            raise ValueError("controlnet is not part of the pipeline classes (use paint_with_words or paint_with_words_batch)")
        check_prompt_chunks(self.max_prompt_chunks)
        check_negative_context(self.negative_color_context, self.negative_strength)
        check_region_prompts(self.region_prompts, self.region_base_weight, self.region_feather, self.negative_color_context)
        unet = getattr(self, "unet", None)
        return check_loras(self.lora, self.region_loras, self.region_prompts, tools=None if unet is None else (None, unet))

    def _check_inputs(self, prompt, height, width, negative_prompt, num_images_per_prompt, generator, latents, callback_steps):
        """The argument block both __call__s share (check_inputs of the diffusers base class, :431) -> (prompt, height, width,
        negative_prompt) as the generation body takes them."""
        height = height or self._default_side()                      # :427-428
        width = width or self._default_side()
        if height % 8 or width % 8:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")
        if not isinstance(prompt, str):
            if not isinstance(prompt, (list, tuple)) or len(prompt) != 1:
                raise ValueError("`prompt` has to be a str (the reference's pipeline generates one image per call)")
            prompt = prompt[0]
        if isinstance(negative_prompt, (list, tuple)):
            negative_prompt = negative_prompt[0] if negative_prompt else ""
        _unused("num_images_per_prompt", num_images_per_prompt, 1)
        _unused("generator", generator, None)
        _unused("latents", latents, None)
        return prompt, height, width, negative_prompt or ""

    def _run(self, start, strength, prompt, color_map_image, color_context, weight_function, num_inference_steps, guidance_scale,
             negative_prompt, seed, output_type, return_dict, callback, callback_steps, loras=None, hold=None):
        """One request through the generation body of the function API, returned as the diffusers pipeline returns it (:821-842). The
        reference calls `callback(i, t, latents)` every `callback_steps` steps (:815-816)."""
        on_step = None if callback is None else (lambda i, t, latents: callback(i, t, latents) if i % callback_steps == 0 else None)
        tools = (self.vae, self.unet, self.text_encoder, self.tokenizer, self.scheduler)
        lat = _generate(tools, str(self.device), [color_context], [color_map_image], [prompt], [seed], num_inference_steps, guidance_scale,
                        weight_function, negative_prompt, start, strength, on_step=on_step, use_region_sigma=False, shared=True,
                        max_prompt_chunks=self.max_prompt_chunks, negative_color_contexts=[self.negative_color_context],
                        negative_strength=self.negative_strength, region_prompts=_region_requests(self.region_prompts, 1),
                        region_base_weight=self.region_base_weight, region_feather=self.region_feather, loras=loras,
                        **({} if hold is None else {"hold": hold}))
        images = _finish(tools, lat, decode=lambda vae, latents: _decode(vae, latents, output_type))
        return SimpleNamespace(images=images, nsfw_content_detected=False) if return_dict else (images, False)

    @torch.no_grad()
    def __call__(
        self,
        prompt: Union[str, List[str]],
        color_map_image: Optional[Image.Image] = None,
        color_context: Dict[Tuple[int, int, int], str] = {},
        weight_function: Callable = lambda w, sigma, qk: 0.1 * w * math.log(sigma + 1) * qk.max(),
        height: Optional[int] = None,
        width: Optional[int] = None,
        num_inference_steps: int = 30,
        guidance_scale: float = 7.5,
        negative_prompt: Optional[Union[str, List[str]]] = "",
        num_images_per_prompt: Optional[int] = 1,
        eta: float = 0.5,
        seed: Optional[int] = 0,
        generator: Optional[torch.Generator] = None,
        image: Optional[Image.Image] = None,
        latents: Optional[torch.FloatTensor] = None,
        output_type: Optional[str] = "pil",
        return_dict: bool = True,
        callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
        callback_steps: Optional[int] = 1,
    ):
        """reference :629-842 (same parameter list, order and defaults). Prompts longer than 75 tokens: `self.max_prompt_chunks`."""
        loras = self._check_extensions()
        held = check_region_strength(self.region_strength, self.region_strength_feather, None if image is None else [image])
        prompt, height, width, negative_prompt = self._check_inputs(prompt, height, width, negative_prompt, num_images_per_prompt, generator,
                                                                    latents, callback_steps)
        hold = _hold_request(held, self.region_strength_feather, eta, num_inference_steps, [color_map_image], [image])
        start, strength = _txt2img_or_img2img([(width, height)], None if image is None else [image], eta)
        if hold is not None:
            start = partial(_held_images, init_images=[image])
        return self._run(start, strength, prompt, color_map_image, color_context, weight_function, num_inference_steps, guidance_scale,
                         negative_prompt, seed, output_type, return_dict, callback, callback_steps, loras=loras, hold=hold)


class PaintWithWord_StableDiffusionInpaintPipeline(PaintWithWord_StableDiffusionPipeline):
    @torch.no_grad()
    def __call__(
        self,
        prompt: Union[str, List[str]],
        image: Image.Image = None,
        mask_image: Optional[Image.Image] = None,
        color_map_image: Optional[Image.Image] = None,
        color_context: Dict[Tuple[int, int, int], str] = {},
        weight_function: Callable = lambda w, sigma, qk: 0.1 * w * math.log(sigma + 1) * qk.max(),
        height: Optional[int] = None,
        width: Optional[int] = None,
        num_inference_steps: int = 30,
        guidance_scale: float = 7.5,
        negative_prompt: Optional[Union[str, List[str]]] = "",
        num_images_per_prompt: Optional[int] = 1,
        eta: float = 1.0,
        seed: Optional[int] = 0,
        generator: Optional[torch.Generator] = None,
        latents: Optional[torch.FloatTensor] = None,
        output_type: Optional[str] = "pil",
        return_dict: bool = True,
        callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
        callback_steps: Optional[int] = 1,
    ):
        """reference paint_with_words_inpaint.py:340-575 (same parameter list, order and defaults). Prompts longer than 75 tokens:
        `self.max_prompt_chunks`."""
        loras = self._check_extensions()
        if self.region_strength or self.region_strength_feather:
            raise ValueError("region_strength / region_strength_feather are not part of the inpaint pipeline (img2img only)")
        if image is None or mask_image is None:
            raise ValueError("`image` and `mask_image` are required for inpainting")
        prompt, height, width, negative_prompt = self._check_inputs(prompt, height, width, negative_prompt, num_images_per_prompt, generator,
                                                                    latents, callback_steps)
        start = partial(_inpaint_start, init_images=[image], mask_images=[mask_image], mask_hw=(height, width), resize_inputs=False)
        return self._run(start, eta, prompt, color_map_image, color_context, weight_function, num_inference_steps, guidance_scale,
                         negative_prompt, seed, output_type, return_dict, callback, callback_steps, loras=loras)
