"""The whole AutoencoderKL encoder (SD configuration) on the native path against the fp32 encoder on the same weights (vaeenc_cases.py), the
switches in a fresh child process, the noise semantics, and the public face: img2img and inpainting with an AutoencoderKLEncDec among the
preloaded tools."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import pww_cases as cases
import vaeenc_cases as C

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SWITCHES = ("PWW_VAE_ENCODE", "PWW_VAE_ENC_HEAD", "PWW_VAE_ENC_DOWN", "PWW_VAE_ENC_TAIL")


@pytest.fixture(scope="module")
def vaes(gpu_device):
    return {dtype: C.make_vae(dtype, gpu_device) for dtype in DTYPES}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("attn", ["1", None], ids=["attn-kernel", "attn-default"])
@pytest.mark.parametrize("shape", C.ENCODE_IMAGES)
def test_encode_against_the_fp32_encoder(gpu_device, vaes, shape, attn, dtype, monkeypatch):
    """Everything native; the mid block's attention kernel with PWW_VAE_ATTN=1, and as the decoder's default has it with nothing set."""
    from pww_hip import vae as V
    from pww_hip import vae_encode as E
    if attn is None:
        monkeypatch.delenv("PWW_VAE_ATTN", raising=False)
    else:
        monkeypatch.setenv("PWW_VAE_ATTN", attn)
    vae = vaes[dtype]
    assert E.covers(vae) and E.enabled()
    st = C.encode_checks(vae, shape, dtype, gpu_device)
    C.assert_native(st, 2, attn=V.attn_enabled(), head=E.head_enabled(), down=E.down_enabled(), tail=E.tail_enabled())
    assert V.attn_enabled() == (attn == "1")


@pytest.mark.parametrize("dtype", DTYPES)
def test_encode_where_the_native_norm_declines(gpu_device, vaes, dtype, monkeypatch):
    """A 40 x 56 image: the 10 x 14 and 5 x 7 levels are no multiple of 8 pixels, the native GroupNorm refuses them, the stock op carries those
    13 norms (down blocks 2 and 3, the mid block), the result is still right, and everything else stays native."""
    from pww_hip import vae_encode as E
    monkeypatch.setenv("PWW_VAE_ATTN", "1")
    st = C.encode_checks(vaes[dtype], C.ODD_IMAGE, dtype, gpu_device)
    C.assert_native(st, 2, head=E.head_enabled(), down=E.down_enabled(), tail=E.tail_enabled(), norms_native=8)
    assert st["group_norm"] == {"native": 2 * 8, "stock": 2 * 13}


def test_the_uint8_image_encodes_to_the_same_bits(gpu_device, vaes):
    from pww_hip import vae_encode as E
    vae = vaes[torch.bfloat16]
    u8 = C.uint8_image(1, 64, 64).to(gpu_device)
    x = C.pixel_table(torch.bfloat16).to(gpu_device)[u8.long()].permute(0, 3, 1, 2).contiguous()
    assert torch.equal(E.encode(vae, u8), E.encode(vae, x))
    with pytest.raises(E.PwwHipError):
        E.encode(vae, x[:, :, :60])
    with pytest.raises(E.PwwHipError):
        E.encode(vae, x, noise=torch.zeros(1, 4, 4, 4))


@pytest.mark.parametrize("switch", ["PWW_VAE_ENC_HEAD", "PWW_VAE_ENC_DOWN", "PWW_VAE_ENC_TAIL"])
def test_a_switch_turns_one_kernel_off(gpu_device, switch):
    """In a fresh process with the switch at 0 the same bars hold (the child asserts them) and the counters move."""
    env = dict(os.environ)
    env.update(PWW_VAE_ENCODE="1", PWW_VAE_ENC_HEAD="1", PWW_VAE_ENC_DOWN="1", PWW_VAE_ENC_TAIL="1", PWW_VAE_ATTN="1")
    env[switch] = "0"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vaeenc_encode_child.py")
    run = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = json.loads([line for line in run.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    part = {"PWW_VAE_ENC_HEAD": "head", "PWW_VAE_ENC_DOWN": "down", "PWW_VAE_ENC_TAIL": "tail"}[switch]
    assert [out[p] for p in ("head", "down", "tail")] == [p != part for p in ("head", "down", "tail")] and len(out["cases"]) == 4
    for case in out["cases"]:
        n = 2 * (3 if part == "down" else 1)
        assert case["stats"][part] == {"native": 0, "stock": n}, case
        for other in {"head", "down", "tail"} - {part}:
            assert case["stats"][other]["stock"] == 0 and case["stats"][other]["native"] > 0, case


def _states(dev):
    return torch.random.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone()


def test_sample_draws_the_noise_as_the_stand_in_does(gpu_device, vaes, monkeypatch):
    """noise="sample" is encode(..., noise=n) for n drawn by the stand-in's recipe from the same generator state, and the CPU and device
    generators are left where the stock `latent_dist.sample()` leaves them."""
    from pww_hip import vae_encode as E
    monkeypatch.setenv("PWW_VAE_ATTN", "1")
    dtype = torch.float16
    vae = vaes[dtype]
    x = C.image((2, 3, 64, 96), dtype, gpu_device)
    torch.manual_seed(5)
    start = _states(gpu_device)
    z = E.encode(vae, x, noise="sample")
    after = _states(gpu_device)
    torch.manual_seed(5)
    n = torch.randn((2, 4, 8, 12), generator=None, device=gpu_device).to(dtype)         # the stand-in's line
    assert torch.equal(E.encode(vae, x, noise=n), z)
    torch.manual_seed(5)
    with torch.no_grad():
        dist = vae.encode(x).latent_dist
        stock = dist.sample()
    stock_after = _states(gpu_device)
    assert torch.equal(after[0], stock_after[0]) and torch.equal(after[1], stock_after[1])
    assert torch.equal(after[0], start[0]) and not torch.equal(after[1], start[1])       # the device generator moved, the CPU one did not
    assert torch.equal(stock, dist.mean + dist.std * n)                                 # (the same n is what the stock line drew)
    # the mode draws nothing
    before = _states(gpu_device)
    E.encode(vae, x)
    assert all(torch.equal(a, b) for a, b in zip(before, _states(gpu_device)))


def _tools(dev, dtype, config="tiny"):
    tools = cases.build_tools(config, dtype=dtype, device=dev)
    return (C.make_vae(dtype, dev),) + tuple(tools[1:])


def test_img2img_encodes_on_the_plug(gpu_device, monkeypatch):
    """End to end: paint_with_words(init_image=...) with an AutoencoderKLEncDec encodes once on the plug; the init latents scheduler.add_noise
    sees are the plug's output bit for bit; with PWW_VAE_ENCODE=0 they are those of the stock line bit for bit and the plug is not entered;
    the noise handed to add_noise is the same bits either way: the random streams did not move."""
    import paint_with_words as pw
    from pww_hip import vae_encode as E
    from gpu_util import uninstall_all
    dtype = torch.float16
    tools = _tools(gpu_device, dtype)
    vae, scheduler = tools[0], tools[4]
    seen, plug, stock = [], [], []
    add_noise, encode, vae_encode = scheduler.add_noise, E.encode, vae.encode

    def spy_add_noise(latents, noise, timesteps):
        seen.append((latents.clone(), noise.clone()))
        return add_noise(latents, noise, timesteps)

    def spy_plug(*a, **kw):
        plug.append((a, kw, encode(*a, **kw)))
        return plug[-1][2]

    def spy_stock(x):
        out = vae_encode(x)
        sample = out.latent_dist.sample

        def record(generator=None):
            stock.append(sample(generator))
            return stock[-1]

        out.latent_dist.sample = record
        return out

    monkeypatch.setattr(scheduler, "add_noise", spy_add_noise, raising=False)
    monkeypatch.setattr(E, "encode", spy_plug)
    monkeypatch.setattr(vae, "encode", spy_stock, raising=False)
    rgb = np.asarray(Image.fromarray(cases.load_example_rgb()).resize((256, 256), Image.NEAREST))
    init = Image.fromarray(cases.synthetic_init_image(256, 3))
    kw = dict(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=cases.RUNNER_PROMPT, num_inference_steps=2,
              guidance_scale=7.5, seed=0, device="cuda:0", preloaded_utils=tools, init_image=init, strength=0.5, return_latents=True)
    try:
        E.reset_stats()
        torch.manual_seed(123)
        lat1 = pw.paint_with_words(**kw)
        st = E.stats()
        assert st["encodes"] == 1 and st["head"] == {"native": 1, "stock": 0} and st["tail"] == {"native": 1, "stock": 0} and st["down"]["native"] == 3
        assert len(plug) == 1 and len(stock) == 0 and len(seen) == 1
        (args, kwargs, z) = plug[0]
        # the uint8 pixels went in, the noise was asked for as the stand-in draws it
        assert args[0] is vae and args[1].dtype == torch.uint8 and tuple(args[1].shape) == (1, 256, 256, 3) and kwargs == {"noise": "sample"}
        assert z.dtype == torch.float32 and tuple(z.shape) == (1, 4, 32, 32) and torch.equal(seen[0][0], z)
        monkeypatch.setenv("PWW_VAE_ENCODE", "0")
        E.reset_stats()
        torch.manual_seed(123)
        lat0 = pw.paint_with_words(**kw)
        assert E.stats()["encodes"] == 0 and len(plug) == 1 and len(stock) == 1 and len(seen) == 2
        assert torch.equal(seen[1][0], (0.18215 * stock[0]).float())                    # the stock line, restated on what ITS call returned
        assert torch.equal(seen[1][1], seen[0][1])                                      # the noise: the same bits
    finally:
        uninstall_all()
    assert tuple(lat1.shape) == tuple(lat0.shape) == (1, 4, 32, 32) and torch.isfinite(lat1).all()
    print("img2img init latents native vs stock: max diff %.3e (max|stock| %.3e)" % ((seen[0][0] - seen[1][0]).abs().max().item(), seen[1][0].abs().max().item()))


def test_every_inpaint_call_site_encodes_on_the_plug(gpu_device):
    """One inpainting request encodes the init image and the masked image; prepare_mask_latents is the third call site."""
    import paint_with_words as pw
    from pww_hip import vae_encode as E
    from gpu_util import uninstall_all
    inpaint = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    dtype = torch.float16
    tools = _tools(gpu_device, dtype, "tiny_inpaint")
    size = (256, 256)
    au = Image.fromarray(cases.load_aurora_rgb()).resize(size, Image.NEAREST)
    mask = cases.load_moon_mask().resize(size, Image.NEAREST)
    init = Image.fromarray(cases.synthetic_init_image(256))
    E.reset_stats()
    try:
        lat = pw.paint_with_words_inpaint(color_context=dict(cases.INPAINT_CONTEXT), color_map_image=au, mask_image=mask, init_image=init,
                                          input_prompt=cases.AURORA_PROMPT, seed=82, num_inference_steps=2, guidance_scale=7.5, device=str(gpu_device),
                                          weight_function=cases.weight_fn_inpaint, preloaded_utils=tools, return_latents=True, strength=1.0)
    finally:
        uninstall_all()
    assert tuple(lat.shape) == (1, 4, 32, 32) and torch.isfinite(lat).all()
    st = E.stats()
    assert st["encodes"] == 2 and st["tail"] == {"native": 2, "stock": 0} and st["head"] == {"native": 2, "stock": 0}, st
    m, masked = torch.ones(1, 1, 256, 256), C.image((1, 3, 256, 256), dtype, "cpu")
    mask_lat, latent = inpaint.prepare_mask_latents(tools[0], m, masked, 1, 256, 256, dtype, gpu_device, None, True)
    assert E.stats()["encodes"] == 3 and tuple(latent.shape) == (2, 4, 32, 32) and latent.dtype == dtype and tuple(mask_lat.shape) == (2, 1, 32, 32)
