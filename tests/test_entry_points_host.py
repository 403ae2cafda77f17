"""The six public faces -- paint_with_words, paint_with_words_batch, paint_with_words_inpaint, paint_with_words_inpaint_batch and the two
pipeline classes -- driven on the CPU (no GPU): what each of them hands to the conditioning layer and to the sampler, which of the caller's
dicts it strips, and what it returns.

The conditioning layer is the real one (mask launches replaced by the oracle's restatements, `cpu_masks`); text encoder, tokenizer and VAE
are sd_standin's tiny ones; the inpaint preparation launch is restated in torch. `PwWSampler` is replaced by a fake that records what
reaches `sample` and hands the latents back, so nothing here depends on a UNet: the arithmetic of the loop is pinned on the device
(tests/test_loop_gpu.py, tests/test_round2_gpu.py)."""
import importlib
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from host_standins import cpu_masks  # noqa: F401  (fixture)

SIDE = 64                      # color maps
INIT = 128                     # init images / masks of the inpaint faces: the function API resizes color map and mask to this
PROMPT = "a photo of a cat and a dog"
NEG_PROMPT = "blurry, a tree, low quality"
CONTEXT = {(0, 0, 0): "cat,1.0,42", (255, 255, 255): "dog,1.5,-1,2.5"}          # a region seed and a blur sigma: the tails get stripped
STRIPPED = {(0, 0, 0): "cat,1.0", (255, 255, 255): "dog,1.5"}
OTHER = {(0, 0, 0): "dog,0.7,-1,3.0"}
OTHER_STRIPPED = {(0, 0, 0): "dog,0.7"}
NEG = {(13, 255, 0): "a tree,1.0,-1,2.5"}
NEG_STRIPPED = {(13, 255, 0): "a tree,1.0"}
words = lambda n: " ".join("word%d" % i for i in range(n))      # noqa: E731  (one token per word: 100 words need 2 chunks, 160 need 3)


def _color_map(side=SIDE):
    img = np.zeros((side, side, 3), dtype=np.uint8)                 # left half (0, 0, 0), right half white, a green square in the middle
    img[:, side // 2:] = 255
    img[side * 3 // 8:side * 5 // 8, side * 3 // 8:side * 5 // 8] = (13, 255, 0)
    return Image.fromarray(img)


def _init_image(side=INIT):
    return Image.fromarray((np.arange(side * side * 3) % 251).astype(np.uint8).reshape(side, side, 3))


def _mask(side=SIDE):
    m = np.zeros((side, side), dtype=np.uint8)
    m[: side // 2] = 255
    return Image.fromarray(m)


class _UNet(torch.nn.Module):
    """What the entry points read off a UNet: `in_channels`, the dtype of its parameters, a `__dict__` to keep samplers in."""
    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.weight = torch.nn.Parameter(torch.zeros(1), requires_grad=False)


def _tools(in_channels=4):
    from sd_standin import HashTokenizer, TinyTextEncoder, TinyVAE, LMSDiscreteScheduler
    sch = LMSDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    return TinyVAE(4, seed=1236), _UNet(in_channels), TinyTextEncoder(32, seed=1235), HashTokenizer(), sch


@pytest.fixture
def rig(cpu_masks, monkeypatch):      # noqa: F811
    """The three modules with the recorders in place. rig.encodes: the bound arguments of every _encode_text_color_inputs call;
    rig.events: ("new" | "sample" | "checked" | "check_errors", sampler) in order; rig.stripped: the dicts handed to
    _extract_seed_and_sigma_from_context by the entry points themselves; rig.prep: the mask shapes the inpaint preparation saw."""
    from pww_hip import ops
    pw = importlib.import_module("paint_with_words.paint_with_words")
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    pipes = importlib.import_module("paint_with_words.pipelines")
    r = SimpleNamespace(pw=pw, inp=inp, pipes=pipes, encodes=[], events=[], stripped=[], prep=[])
    real_encode, real_extract = pw._encode_text_color_inputs, pw._extract_seed_and_sigma_from_context
    params = inspect.signature(real_encode)

    def encode(*args, **kw):
        bound = params.bind(*args, **kw)
        bound.apply_defaults()
        r.encodes.append(dict(bound.arguments, color_context_before=dict(bound.arguments["color_context"])))
        return real_encode(*args, **kw)

    def extract(ctx, *args, **kw):
        r.stripped.append(ctx)
        return real_extract(ctx, *args, **kw)

    class Sampler:
        def __init__(self, unet, scheduler, mode):
            self.mode, self.calls = mode, []
            r.events.append(("new", self))

        def sample(self, cond, uncond, latents, timesteps, guidance_scale, weight_function, extra_channels=None, on_step=None, negative_strength=1.0):
            self.calls.append(SimpleNamespace(cond=cond, uncond=uncond, latents=latents, timesteps=timesteps, guidance_scale=guidance_scale,
                                              extra_channels=extra_channels, on_step=on_step, negative_strength=negative_strength))
            r.events.append(("sample", self))
            if on_step is not None:
                for i, t in enumerate(timesteps):
                    on_step(i, t, latents)
            return latents

        def checked(self, latents):
            r.events.append(("checked", self))
            return latents

        def check_errors(self):
            r.events.append(("check_errors", self))

    def inpaint_prep(rgb, mask, lat_h, lat_w):      # ops.inpaint_prep restated: (mask, masked image, latent-size mask)
        r.prep.append(tuple(mask.shape))
        m = (mask.float() / 255.0 >= 0.5).float()[None, None]
        pix = rgb.permute(2, 0, 1)[None].float() / 127.5 - 1.0
        return m, pix * (m < 0.5), torch.nn.functional.interpolate(m, size=(lat_h, lat_w))

    for mod in (pw, inp):       # (a module that imported the name from the function-API module holds its own reference)
        monkeypatch.setattr(mod, "_encode_text_color_inputs", encode, raising=False)
        monkeypatch.setattr(mod, "_extract_seed_and_sigma_from_context", extract, raising=False)
    monkeypatch.setattr(pw, "PwWSampler", Sampler)
    monkeypatch.setattr(ops, "inpaint_prep", inpaint_prep)
    monkeypatch.setattr(pw, "DEFAULT_MODE", "eager")
    r.count = lambda kind: sum(1 for k, _ in r.events if k == kind)
    r.last = lambda: [s for k, s in r.events if k == "sample"][-1].calls[-1]
    r.kw = lambda tools, **kw: dict(dict(device="cpu", preloaded_utils=tools, num_inference_steps=3, unconditional_input_prompt=NEG_PROMPT), **kw)
    return r


def _encode_args(call):
    return (call["use_sigma"], call["max_prompt_chunks"], call["min_prompt_chunks"], call["negative_maps"])


# ---- paint_with_words ----------------------------------------------------------------------------------------------------------------------

def test_paint_with_words(rig):
    tools = _tools()
    ctx, neg = dict(CONTEXT), dict(NEG)
    lat = rig.pw.paint_with_words(ctx, _color_map(), PROMPT, seed=3, negative_color_context=neg, negative_strength=0.5, return_latents=True,
                                  **rig.kw(tools))
    assert len(rig.encodes) == 1 and _encode_args(rig.encodes[0]) == (True, 1, 1, True)
    e = rig.encodes[0]
    assert e["color_context"] is ctx and e["negative_color_context"] is neg and e["color_map_image"].size == (SIDE, SIDE)
    assert e["input_prompt"] == PROMPT and e["unconditional_input_prompt"] == NEG_PROMPT and e["dtype"] == torch.float32 and e["device"] == "cpu"
    assert ctx == STRIPPED and neg == NEG_STRIPPED and rig.stripped == []       # (stripped by the conditioning layer itself)
    s = rig.last()
    assert isinstance(s.cond, dict) and isinstance(s.uncond, dict) and tuple(s.cond["CONTEXT_TENSOR"].shape) == (1, 77, 32)
    assert tuple(s.latents.shape) == (1, 4, 8, 8) and len(s.timesteps) == 3 and s.extra_channels is None
    assert s.negative_strength == 0.5 and s.guidance_scale == 7.5 and s.on_step is None
    assert lat is s.latents and rig.count("checked") == 1 and rig.count("check_errors") == 0
    # the region seed (42, left half) reached the initial latent: it differs from the plain seed-3 latent there, and only there
    plain = torch.randn((1, 4, 8, 8), generator=torch.manual_seed(3)) * tools[4].init_noise_sigma
    assert torch.equal(s.latents[..., 5:], plain[..., 5:]) and not torch.equal(s.latents[..., :3], plain[..., :3])
    # decoded: one PIL image, one check_errors; no negative context: the reference's unconditional pass
    img = rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, **rig.kw(tools))
    assert isinstance(img, Image.Image) and img.size == (SIDE, SIDE) and rig.count("check_errors") == 1 and rig.count("checked") == 1
    assert rig.encodes[1]["negative_color_context"] is None and rig.encodes[1]["negative_maps"] is False and rig.last().negative_strength == 1.0
    # img2img: strength 0.5 at 4 steps keeps the last 2 timesteps; the latent comes from the init image (rounded down to a multiple of 32)
    rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, init_image=_init_image(100), strength=0.5, return_latents=True,
                            **rig.kw(tools, num_inference_steps=4))
    s = rig.last()
    assert len(s.timesteps) == 2 and torch.equal(s.timesteps, tools[4].timesteps[2:]) and tuple(s.latents.shape) == (1, 4, 12, 12)
    assert s.extra_channels is None
    # chunks: the larger of what the prompt and the unconditional prompt need under the cap
    rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, max_prompt_chunks=3, return_latents=True,
                            **rig.kw(tools, unconditional_input_prompt=words(160)))
    assert _encode_args(rig.encodes[-1]) == (True, 3, 3, False) and tuple(rig.last().cond["CONTEXT_TENSOR"].shape) == (1, 231, 32)
    with pytest.raises(AttributeError):
        rig.pw.paint_with_words(dict(CONTEXT), None, PROMPT, **rig.kw(tools))       # the reference dereferences the color map unconditionally


# ---- paint_with_words_batch ----------------------------------------------------------------------------------------------------------------

def test_batch_with_everything_shared(rig):
    tools = _tools()
    ctx, neg = dict(CONTEXT), dict(NEG)
    lat = rig.pw.paint_with_words_batch(ctx, _color_map(), PROMPT, [0, 1, 2], negative_color_context=neg, negative_strength=2.0,
                                        return_latents=True, **rig.kw(tools))
    assert len(rig.encodes) == 1 and _encode_args(rig.encodes[0]) == (True, 1, 1, True)
    assert rig.encodes[0]["color_context"] is ctx and rig.encodes[0]["negative_color_context"] is neg
    assert ctx == STRIPPED and neg == NEG_STRIPPED and rig.stripped == []
    s = rig.last()
    assert isinstance(s.cond, dict) and isinstance(s.uncond, dict) and tuple(s.latents.shape) == (3, 4, 8, 8) and len(s.timesteps) == 3
    assert s.negative_strength == 2.0 and s.extra_channels is None and lat is s.latents
    assert not torch.equal(lat[0], lat[1]) and rig.count("checked") == 1 and rig.count("check_errors") == 0
    images = rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1], **rig.kw(tools))
    assert len(images) == 2 and all(isinstance(im, Image.Image) and im.size == (SIDE, SIDE) for im in images)
    assert rig.count("check_errors") == 1 and rig.count("checked") == 1


def test_batch_with_per_request_values(rig):
    tools = _tools()
    a, b, neg = dict(CONTEXT), dict(OTHER), dict(NEG)
    lat = rig.pw.paint_with_words_batch([a, a, b], _color_map(), PROMPT, [5, 6, 7], negative_color_context=[None, neg, None],
                                        init_images=_init_image(SIDE), strength=0.5, return_latents=True, **rig.kw(tools, num_inference_steps=4))
    assert len(rig.encodes) == 3 and all(_encode_args(e) == (True, 1, 1, True) for e in rig.encodes)      # negative_maps: over all requests
    assert [e["color_context_before"] for e in rig.encodes] == [CONTEXT, CONTEXT, OTHER]                   # private copies, tails still on
    assert all(e["color_context"] is not a and e["color_context"] is not b for e in rig.encodes)
    got_negs = [e["negative_color_context"] for e in rig.encodes]
    assert got_negs[0] is None and got_negs[2] is None and got_negs[1] is not neg and got_negs[1] == NEG_STRIPPED
    # the caller's dicts are stripped afterwards, each object once: color contexts and negative contexts
    assert a == STRIPPED and b == OTHER_STRIPPED and neg == NEG_STRIPPED
    assert sorted(map(id, rig.stripped)) == sorted(map(id, (a, b, neg)))
    s = rig.last()
    assert isinstance(s.cond, list) and isinstance(s.uncond, list) and len(s.cond) == len(s.uncond) == 3
    assert tuple(s.latents.shape) == (3, 4, 8, 8) and len(s.timesteps) == 2 and lat is s.latents
    # one negative dict object serving two requests is stripped once
    rig.stripped.clear()
    neg2 = dict(NEG)
    rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1, 2], negative_color_context=[neg2, None, neg2],
                                  return_latents=True, **rig.kw(tools))
    assert neg2 == NEG_STRIPPED and sum(1 for c in rig.stripped if c is neg2) == 1 and len(rig.encodes) == 6


def test_batch_prompts_that_need_different_chunk_counts(rig):
    tools = _tools()
    prompts = [PROMPT, words(100) + " a cat", PROMPT]
    rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), prompts, [0, 1, 2], max_prompt_chunks=3, return_latents=True,
                                  **rig.kw(tools, unconditional_input_prompt=""))
    assert len(rig.encodes) == 3 and all(_encode_args(e) == (True, 3, 2, False) for e in rig.encodes)
    assert [e["input_prompt"] for e in rig.encodes] == prompts
    assert all(tuple(c["CONTEXT_TENSOR"].shape) == (1, 154, 32) for c in rig.last().cond)
    # shared: the first prompt and the unconditional prompt decide
    rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1], max_prompt_chunks=3, return_latents=True,
                                  **rig.kw(tools, unconditional_input_prompt=words(100)))
    assert len(rig.encodes) == 4 and _encode_args(rig.encodes[-1]) == (True, 3, 2, False)


def test_batch_argument_checks_and_the_empty_batch(rig, monkeypatch):
    def no_tools(*a, **kw):
        raise AssertionError("the tools were touched")
    for mod in (rig.pw, rig.inp):
        monkeypatch.setattr(mod, "pww_load_tools", no_tools, raising=False)
    assert rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, []) == []
    assert rig.inp.paint_with_words_inpaint_batch(dict(CONTEXT), _color_map(), _mask(), _init_image(), PROMPT, []) == []
    assert rig.events == [] and rig.encodes == []
    tools = _tools()
    with pytest.raises(ValueError, match="paint_with_words_batch: all color maps of one call must have the same size"):
        rig.pw.paint_with_words_batch(dict(CONTEXT), [_color_map(), _color_map(96)], PROMPT, [0, 1], **rig.kw(tools))
    with pytest.raises(ValueError, match="paint_with_words_inpaint_batch: all init images of one call must have the same size"):
        rig.inp.paint_with_words_inpaint_batch(dict(CONTEXT), _color_map(), _mask(), [_init_image(), _init_image(96)], PROMPT, [0, 1],
                                               **rig.kw(_tools(9)))
    with pytest.raises(ValueError, match="input_prompts has 3 entries for 2 requests"):
        rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), [PROMPT] * 3, [0, 1], **rig.kw(tools))
    with pytest.raises(ValueError, match="mask_images has 1 entries for 2 requests"):
        rig.inp.paint_with_words_inpaint_batch(dict(CONTEXT), _color_map(), [_mask()], _init_image(), PROMPT, [0, 1], **rig.kw(_tools(9)))
    assert rig.events == [] and rig.encodes == []


# ---- paint_with_words_inpaint / _batch -----------------------------------------------------------------------------------------------------

def test_inpaint(rig):
    tools = _tools(9)
    ctx, neg = dict(CONTEXT), dict(NEG)
    lat = rig.inp.paint_with_words_inpaint(ctx, _color_map(), _mask(), _init_image(), PROMPT, seed=4, negative_color_context=neg,
                                           negative_strength=0.5, return_latents=True, **rig.kw(tools))
    assert len(rig.encodes) == 1 and _encode_args(rig.encodes[0]) == (True, 1, 1, True)
    e = rig.encodes[0]
    assert e["color_map_image"].size == (INIT, INIT) and rig.prep == [(INIT, INIT)]      # color map and mask resized to the init image
    assert np.array_equal(np.asarray(e["color_map_image"]), np.asarray(_color_map().resize((INIT, INIT), Image.NEAREST)))
    assert e["color_context"] is ctx and e["negative_color_context"] is neg and ctx == STRIPPED and neg == NEG_STRIPPED
    s = rig.last()
    assert isinstance(s.cond, dict) and tuple(s.latents.shape) == (1, 4, 16, 16) and tuple(s.extra_channels.shape) == (1, 5, 16, 16)
    assert len(s.timesteps) == 3 and s.negative_strength == 0.5 and lat is s.latents           # strength defaults to 1.0: every step
    assert set(s.extra_channels[:, 0].unique().tolist()) == {0.0, 1.0}                          # the latent-size mask leads the extra channels
    assert rig.count("checked") == 1 and rig.count("check_errors") == 0
    img = rig.inp.paint_with_words_inpaint(dict(CONTEXT), _color_map(), _mask(), _init_image(), PROMPT, strength=0.5,
                                           **rig.kw(tools, num_inference_steps=4))
    assert isinstance(img, Image.Image) and img.size == (INIT, INIT) and rig.count("check_errors") == 1 and rig.count("checked") == 1
    assert len(rig.last().timesteps) == 2 and rig.encodes[-1]["negative_maps"] is False
    rig.inp.paint_with_words_inpaint(dict(CONTEXT), _color_map(), _mask(), _init_image(), PROMPT, max_prompt_chunks=2, return_latents=True,
                                     **rig.kw(tools, unconditional_input_prompt=words(160)))
    assert _encode_args(rig.encodes[-1]) == (True, 2, 2, False)
    with pytest.raises(ValueError, match="Incorrect configuration settings! .* expects 4 input channels but received 4 latent \\+ 1 mask \\+ 4"):
        rig.inp.paint_with_words_inpaint(dict(CONTEXT), _color_map(), _mask(), _init_image(), PROMPT, **rig.kw(_tools(4)))


def test_inpaint_batch(rig):
    tools = _tools(9)
    ctx, neg = dict(CONTEXT), dict(NEG)
    rig.inp.paint_with_words_inpaint_batch(ctx, _color_map(), [_mask(), _mask(INIT)], _init_image(), PROMPT, [0, 1], negative_color_context=neg,
                                           return_latents=True, **rig.kw(tools))
    assert len(rig.encodes) == 1 and _encode_args(rig.encodes[0]) == (True, 1, 1, True)        # masks and init images do not split the conditioning
    assert rig.encodes[0]["color_context"] is ctx and ctx == STRIPPED and neg == NEG_STRIPPED and rig.stripped == []
    assert rig.encodes[0]["color_map_image"].size == (INIT, INIT) and rig.prep == [(INIT, INIT)] * 2
    s = rig.last()
    assert isinstance(s.cond, dict) and tuple(s.latents.shape) == (2, 4, 16, 16) and tuple(s.extra_channels.shape) == (2, 5, 16, 16)
    assert rig.count("checked") == 1 and rig.count("check_errors") == 0
    # per-request values: private copies are parsed; afterwards this function strips the caller's NEGATIVE dicts only (each object once),
    # where paint_with_words_batch strips the color contexts too
    a, b, neg = dict(CONTEXT), dict(OTHER), dict(NEG)
    images = rig.inp.paint_with_words_inpaint_batch([a, a, b], _color_map(), _mask(), _init_image(), PROMPT, [5, 6, 7],
                                                    negative_color_context=[neg, None, neg], strength=0.5, **rig.kw(tools, num_inference_steps=4))
    assert len(rig.encodes) == 4 and all(_encode_args(e) == (True, 1, 1, True) for e in rig.encodes[1:])
    assert [e["color_context_before"] for e in rig.encodes[1:]] == [CONTEXT, CONTEXT, OTHER]
    assert all(e["color_context"] is not a and e["color_context"] is not b and e["negative_color_context"] is not neg for e in rig.encodes[1:])
    assert all(e["color_map_image"].size == (INIT, INIT) for e in rig.encodes[1:])
    assert a == CONTEXT and b == OTHER and neg == NEG_STRIPPED and [id(c) for c in rig.stripped] == [id(neg)]
    s = rig.last()
    assert isinstance(s.cond, list) and len(s.cond) == len(s.uncond) == 3 and len(s.timesteps) == 2
    assert tuple(s.latents.shape) == (3, 4, 16, 16) and tuple(s.extra_channels.shape) == (3, 5, 16, 16)
    assert len(images) == 3 and all(im.size == (INIT, INIT) for im in images) and rig.count("check_errors") == 1 and rig.count("checked") == 1
    # different chunk counts under the cap
    rig.inp.paint_with_words_inpaint_batch(dict(CONTEXT), _color_map(), _mask(), _init_image(), [PROMPT, words(100)], [0, 1], max_prompt_chunks=3,
                                           return_latents=True, **rig.kw(tools, unconditional_input_prompt=""))
    assert all(_encode_args(e) == (True, 3, 2, False) for e in rig.encodes[-2:])


# ---- the pipeline classes ------------------------------------------------------------------------------------------------------------------

def _pipe(rig, inpaint=False):
    vae, unet, text, tok, sch = _tools(9 if inpaint else 4)
    cls = rig.pipes.PaintWithWord_StableDiffusionInpaintPipeline if inpaint else rig.pipes.PaintWithWord_StableDiffusionPipeline
    return cls(vae, text, tok, unet, sch)


def test_pipeline(rig):
    pipe = _pipe(rig)
    pipe.max_prompt_chunks, pipe.negative_color_context, pipe.negative_strength = 2, dict(NEG), 0.25
    ctx, calls = dict(CONTEXT), []
    out = pipe([PROMPT], _color_map(), ctx, height=96, width=64, num_inference_steps=4, negative_prompt=[NEG_PROMPT], seed=3, output_type="np",
               callback=lambda i, t, lat: calls.append(i), callback_steps=2)
    assert len(rig.encodes) == 1 and _encode_args(rig.encodes[0]) == (False, 2, 1, True)            # the class parses the blur sigma and drops it
    e = rig.encodes[0]
    assert e["color_context"] is ctx and ctx == STRIPPED and pipe.negative_color_context == NEG_STRIPPED
    assert e["input_prompt"] == PROMPT and e["unconditional_input_prompt"] == NEG_PROMPT and e["color_map_image"].size == (SIDE, SIDE)
    s = rig.last()
    assert isinstance(s.cond, dict) and tuple(s.latents.shape) == (1, 4, 12, 8) and len(s.timesteps) == 4      # height / width size the latent
    assert s.extra_channels is None and s.negative_strength == 0.25 and calls == [0, 2]
    assert isinstance(out.images, np.ndarray) and out.images.shape == (1, 96, 64, 3) and out.images.dtype == np.float32
    assert 0.0 <= float(out.images.min()) and float(out.images.max()) <= 1.0 and out.nsfw_content_detected is False
    assert rig.count("check_errors") == 1 and rig.count("checked") == 0
    # img2img through `image` / `eta`; return_dict=False; no callback: no on_step
    pipe.negative_color_context = None
    got = pipe(PROMPT, _color_map(), dict(CONTEXT), height=64, width=64, num_inference_steps=4, eta=0.5, image=_init_image(SIDE), return_dict=False)
    assert isinstance(got, tuple) and got[1] is False and len(got[0]) == 1 and got[0][0].size == (SIDE, SIDE)
    s = rig.last()
    assert len(s.timesteps) == 2 and s.on_step is None and s.negative_strength == 0.25 and rig.count("check_errors") == 2
    assert rig.encodes[-1]["negative_maps"] is False and rig.encodes[-1]["unconditional_input_prompt"] == ""
    # the argument block
    n = len(rig.encodes)
    with pytest.raises(ValueError, match="`height` and `width` have to be divisible by 8 but are 60 and 64"):
        pipe(PROMPT, _color_map(), dict(CONTEXT), height=60, width=64)
    for steps in (0, None, 1.5):
        with pytest.raises(ValueError, match="`callback_steps` has to be a positive integer"):
            pipe(PROMPT, _color_map(), dict(CONTEXT), height=64, width=64, callback_steps=steps)
    with pytest.raises(ValueError, match="`prompt` has to be a str"):
        pipe([PROMPT, PROMPT], _color_map(), dict(CONTEXT), height=64, width=64)
    pipe.max_prompt_chunks = 4
    with pytest.raises(ValueError, match="max_prompt_chunks"):
        pipe(PROMPT, _color_map(), dict(CONTEXT), height=64, width=64)
    assert len(rig.encodes) == n


def test_inpaint_pipeline(rig):
    pipe = _pipe(rig, inpaint=True)
    pipe.negative_color_context = dict(NEG)
    calls = []
    out = pipe(PROMPT, _init_image(), _mask(INIT), _color_map(), dict(CONTEXT), height=INIT, width=INIT, num_inference_steps=4,
               negative_prompt=NEG_PROMPT, seed=4, output_type="np", callback=lambda i, t, lat: calls.append(i), callback_steps=3)
    assert len(rig.encodes) == 1 and _encode_args(rig.encodes[0]) == (False, 1, 1, True)
    assert rig.encodes[0]["color_map_image"].size == (SIDE, SIDE) and rig.prep == [(INIT, INIT)]        # taken as given: no resize to `image`
    s = rig.last()
    assert isinstance(s.cond, dict) and tuple(s.latents.shape) == (1, 4, 16, 16) and tuple(s.extra_channels.shape) == (1, 5, 16, 16)
    assert len(s.timesteps) == 4 and calls == [0, 3] and s.negative_strength == 1.0                     # eta defaults to 1.0: every step
    assert out.images.shape == (1, INIT, INIT, 3) and rig.count("check_errors") == 1 and rig.count("checked") == 0
    got = pipe(PROMPT, _init_image(), _mask(INIT), _color_map(), dict(CONTEXT), height=INIT, width=INIT, num_inference_steps=4, eta=0.5,
               return_dict=False)
    assert got[1] is False and got[0][0].size == (INIT, INIT) and len(rig.last().timesteps) == 2 and rig.count("check_errors") == 2
    n = len(rig.events)
    with pytest.raises(ValueError, match="`height` x `width` = 64 x 64 gives a \\(8, 8\\) latent mask but `image` gives \\(16, 16\\) latents"):
        pipe(PROMPT, _init_image(), _mask(INIT), _color_map(), dict(CONTEXT), height=SIDE, width=SIDE, num_inference_steps=2)
    with pytest.raises(AssertionError, match="Image and Mask must have the same spatial dimensions"):
        pipe(PROMPT, _init_image(), _mask(SIDE), _color_map(), dict(CONTEXT), height=INIT, width=INIT, num_inference_steps=2)   # the mask is not resized either
    with pytest.raises(ValueError, match="`image` and `mask_image` are required for inpainting"):
        pipe(PROMPT, None, _mask(INIT), _color_map(), dict(CONTEXT), height=INIT, width=INIT)
    with pytest.raises(ValueError, match="`image` and `mask_image` are required for inpainting"):      # in front of the shared argument block
        pipe(PROMPT, _init_image(), None, height=60, width=64)
    with pytest.raises(ValueError, match="`height` and `width` have to be divisible by 8 but are 60 and 64"):
        pipe(PROMPT, _init_image(), _mask(INIT), height=60, width=64)
    assert len(rig.events) == n                                                                        # none of them reached the sampler


# ---- the execution mode is read at call time -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("face", ["function", "inpaint", "pipeline", "inpaint_pipeline"])
def test_default_mode_is_read_at_call_time(rig, face):
    if face == "function":
        tools = _tools()
        call = lambda: rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, **rig.kw(tools, num_inference_steps=2))      # noqa: E731
    elif face == "inpaint":
        tools = _tools(9)
        call = lambda: rig.inp.paint_with_words_inpaint_batch(dict(CONTEXT), _color_map(), _mask(), _init_image(SIDE), PROMPT, [0, 1],      # noqa: E731
                                                              **rig.kw(tools, num_inference_steps=2))
    else:
        pipe = _pipe(rig, inpaint=face == "inpaint_pipeline")
        args = (_init_image(SIDE), _mask()) if face == "inpaint_pipeline" else ()
        call = lambda: pipe(PROMPT, *args, color_map_image=_color_map(), color_context=dict(CONTEXT), height=SIDE, width=SIDE,      # noqa: E731
                            num_inference_steps=2)
    for mode in ("eager", "folded", "eager"):
        rig.pw.DEFAULT_MODE = mode
        del rig.events[:]
        call()
        used = [(kind, s.mode) for kind, s in rig.events if kind != "new"]
        assert used == [("sample", mode), ("check_errors", mode)], (face, mode, used)      # the loop and the tail, on the same sampler
    assert len({id(s) for _, s in rig.events}) == 1 and rig.count("new") == 0                # the first mode's sampler was kept
