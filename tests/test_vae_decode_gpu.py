"""The whole AutoencoderKL decoder (SD configuration) on the native path against the fp32 decoder on the same weights (vae_cases.py), the
switches in a fresh child process, and the public face: paint_with_words with an AutoencoderKL among the preloaded tools."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pww_cases as cases
import vae_cases as C

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def vaes(gpu_device):
    return {dtype: C.make_vae(dtype, gpu_device) for dtype in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", C.DECODE_LATENTS)
def test_decode_against_the_fp32_decoder(gpu_device, vaes, shape, dtype, monkeypatch):
    """Everything native: the attention kernel is off by default (profiles/vae_decode.md), PWW_VAE_ATTN=1 turns it on."""
    from pww_hip import vae as V
    monkeypatch.setenv("PWW_VAE_ATTN", "1")
    monkeypatch.delenv("PWW_VAE_TAIL", raising=False)
    vae = vaes[dtype]
    assert V.covers(vae) and V.attn_enabled() and V.tail_enabled()
    st = C.decode_checks(vae, shape, dtype, gpu_device)
    C.assert_native(st, 2)
    assert st["proj_attn"]["native"] + st["proj_attn"]["stock"] == 2


def test_decode_with_the_default_switches(gpu_device, vaes, monkeypatch):
    """Nothing set: the tail native, the attention on the stock sequence; the same bars."""
    from pww_hip import vae as V
    monkeypatch.delenv("PWW_VAE_ATTN", raising=False)
    monkeypatch.delenv("PWW_VAE_TAIL", raising=False)
    assert not V.attn_enabled() and V.tail_enabled()
    st = C.decode_checks(vaes[torch.bfloat16], C.DECODE_LATENTS[1], torch.bfloat16, gpu_device)
    C.assert_native(st, 2, attn=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_where_the_native_norm_declines(gpu_device, vaes, dtype, monkeypatch):
    """h w = 35 at the coarsest level is no multiple of 8: the native GroupNorm refuses it there and one level up (140), the stock ops carry
    those norms, the result is still right, and stats() shows it."""
    from pww_hip import vae as V
    monkeypatch.setenv("PWW_VAE_ATTN", "1")
    monkeypatch.delenv("PWW_VAE_TAIL", raising=False)
    vae = vaes[dtype]
    z = C.latent(C.ODD_LATENT, dtype, gpu_device)
    with torch.no_grad():
        ref, stock = C.decode_reference(vae, z), vae.decode(z).sample
    V.reset_stats()
    sample, u8 = V.decode(vae, z, "sample"), V.decode(vae, z, "uint8")
    st = V.stats()
    what = "decode %s %s" % (C.ODD_LATENT, str(dtype).split(".")[-1])
    assert tuple(sample.shape) == (1, 3, 40, 56)
    eps = C.check_sample(sample, stock, ref, what)
    C.check_uint8(u8, ref, eps, what)
    # the mid block (2 resnets + the attention's norm) and up block 0 (3 resnets) at 5 x 7, up block 1 at 10 x 14: 2 * 8 + 1 norms per decode
    assert st["group_norm"] == {"native": 2 * 12, "stock": 2 * 17}, st
    assert st["conv3x3"]["stock"] == 0 and st["upsample"] == {"native": 6, "stock": 0} and st["tail"] == {"native": 2, "stock": 0}, st
    assert st["attention"] == {"native": 2, "stock": 0}, st


@pytest.mark.parametrize("switch", ["PWW_VAE_ATTN", "PWW_VAE_TAIL"])
def test_a_switch_turns_one_kernel_off(gpu_device, switch):
    """In a fresh process with the switch at 0 the same bars hold (the child asserts them) and the counters move."""
    env = dict(os.environ)
    env.update(PWW_VAE_ATTN="1", PWW_VAE_TAIL="1")      # (the attention kernel is off unless asked for)
    env[switch] = "0"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vae_decode_child.py")
    run = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = json.loads([line for line in run.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert out["attn"] == (switch != "PWW_VAE_ATTN") and out["tail"] == (switch != "PWW_VAE_TAIL") and len(out["cases"]) == 4
    part = "attention" if switch == "PWW_VAE_ATTN" else "tail"
    other = "tail" if part == "attention" else "attention"
    for case in out["cases"]:
        assert case["stats"][part] == {"native": 0, "stock": 2} and case["stats"][other] == {"native": 2, "stock": 0}, case


def _tools(dev, dtype):
    tools = cases.build_tools("tiny", dtype=dtype, device=dev)
    return (C.make_vae(dtype, dev),) + tuple(tools[1:])


def test_paint_with_words_returns_the_uint8_decode(gpu_device, monkeypatch):
    """End to end: the PIL image of paint_with_words is Image.fromarray of the plug's uint8 decode of the final latents, bit for bit; with
    PWW_VAE=0 it is the image of the stock _pil_from_latents code, bit for bit, and the plug is not entered."""
    import paint_with_words as pw
    from PIL import Image
    from pww_hip import vae as V
    mod = importlib.import_module("paint_with_words.paint_with_words")
    dtype = torch.float16
    tools = _tools(gpu_device, dtype)
    seen = []
    orig = mod._pil_from_latents

    def grab(vae, latents, *a, **kw):
        seen.append(latents.clone())
        return orig(vae, latents, *a, **kw)

    monkeypatch.setattr(mod, "_pil_from_latents", grab)
    rgb = np.asarray(Image.fromarray(cases.load_example_rgb()).resize((256, 256), Image.NEAREST))      # 32 x 32 latents: a quick request
    kw = dict(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=cases.RUNNER_PROMPT,
              num_inference_steps=2, guidance_scale=7.5, seed=0, device="cuda:0", preloaded_utils=tools)
    monkeypatch.delenv("PWW_VAE", raising=False)
    monkeypatch.setenv("PWW_VAE_ATTN", "1")
    V.reset_stats()
    image = pw.paint_with_words(**kw)
    h, w = rgb.shape[0] // 8, rgb.shape[1] // 8
    assert isinstance(image, Image.Image) and image.size == (8 * w, 8 * h) and V.stats()["decodes"] == 1 and V.stats()["tail"]["native"] == 1
    latents = seen[-1]
    assert tuple(latents.shape) == (1, 4, h, w)
    z = (latents.clone() / 0.18215).to(dtype)
    want = V.decode(tools[0], z, "uint8")
    assert want.dtype == torch.uint8 and np.array_equal(np.asarray(image), want[0].cpu().numpy())
    # the float output types take the .sample form
    pixels = orig(tools[0], latents, "np")
    sample = V.decode(tools[0], z, "sample")
    assert pixels.dtype == np.float32 and np.array_equal(pixels, (sample / 2 + 0.5).clamp(0, 1).float().cpu().permute(0, 2, 3, 1).numpy())
    # PWW_VAE=0: the stock code, restated here on what ITS call of vae.decode returned (two runs of the stock convolutions need not agree
    # bit for bit, so the restatement does not decode a second time)
    monkeypatch.setenv("PWW_VAE", "0")
    V.reset_stats()
    calls = []
    stock_decode = tools[0].decode

    def spy(arg):
        calls.append((arg.clone(), stock_decode(arg)))
        return calls[-1][1]

    monkeypatch.setattr(tools[0], "decode", spy, raising=False)
    stock_images = orig(tools[0], latents)
    monkeypatch.undo()
    assert V.stats()["decodes"] == 0 and len(calls) == 1 and torch.equal(calls[0][0], z)
    stock_pixels = (calls[0][1].sample / 2 + 0.5).clamp(0, 1).detach().float().cpu().permute(0, 2, 3, 1).numpy()
    assert len(stock_images) == 1 and np.array_equal(np.asarray(stock_images[0]), (stock_pixels * 255).round().astype("uint8")[0])
    diff = np.abs(np.asarray(stock_images[0]).astype(np.int32) - np.asarray(image).astype(np.int32))
    print("native vs stock image: max byte difference %d, mean %.4f" % (diff.max(), diff.mean()))
