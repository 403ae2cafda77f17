"""Host side of the AutoencoderKL encode: the stand-in's layout and its latent_dist, the plug's structural check, the side library's table
rows, a real build with its argument checks, preprocess_uint8, and that a VAE the plug does not cover never enters it. No GPU."""
import ctypes
import importlib
import inspect
import subprocess

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import PKG, REPO


def test_the_stand_in_has_the_diffusers_encoder_layout():
    from sd_standin import AutoencoderKL, AutoencoderKLEncDec
    from sd_standin.vae import VaeMidBlock
    state = torch.random.get_rng_state()
    vae = AutoencoderKLEncDec()
    again = AutoencoderKLEncDec()
    assert torch.equal(torch.random.get_rng_state(), state)                     # the global generator untouched
    assert all(torch.equal(p, q) for p, q in zip(vae.parameters(), again.parameters()))
    assert isinstance(vae, AutoencoderKL) and not any(p.requires_grad for p in vae.parameters())
    base = AutoencoderKL()
    for mine, theirs in ((vae.decoder, base.decoder), (vae.post_quant_conv, base.post_quant_conv)):
        assert all(torch.equal(p, q) for p, q in zip(mine.parameters(), theirs.parameters()))      # the decoder bit for bit
    enc = vae.encoder
    cin = enc.conv_in
    assert (cin.in_channels, cin.out_channels, cin.kernel_size, cin.padding) == (3, 128, (3, 3), (1, 1))
    assert len(enc.down_blocks) == 4 and [len(b.resnets) for b in enc.down_blocks] == [2, 2, 2, 2]
    assert [(b.resnets[0].conv1.in_channels, b.resnets[-1].conv2.out_channels) for b in enc.down_blocks] == [(128, 128), (128, 256), (256, 512), (512, 512)]
    assert [b.resnets[0].conv_shortcut is not None for b in enc.down_blocks] == [False, True, True, False]
    assert all(b.resnets[1].conv_shortcut is None for b in enc.down_blocks) and enc.down_blocks[1].resnets[0].conv_shortcut.kernel_size == (1, 1)
    assert [b.downsamplers is not None for b in enc.down_blocks] == [True, True, True, False]
    for b, ch in zip(enc.down_blocks[:3], (128, 256, 512)):
        conv = b.downsamplers[0].conv
        assert len(b.downsamplers) == 1 and (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) == (ch, ch, (3, 3), (2, 2), (0, 0))
    assert isinstance(enc.mid_block, VaeMidBlock) and enc.mid_block.attentions[0].channels == 512 and enc.mid_block.attentions[0].num_heads == 1
    norms = [m for m in enc.modules() if isinstance(m, nn.GroupNorm)]
    assert len(norms) == 22 and all(m.num_groups == 32 and m.eps == 1e-6 for m in norms)
    assert enc.conv_norm_out.num_channels == 512 and isinstance(enc.conv_act, nn.SiLU)
    assert (enc.conv_out.in_channels, enc.conv_out.out_channels, enc.conv_out.kernel_size, enc.conv_out.padding) == (512, 8, (3, 3), (1, 1))
    qc = vae.quant_conv
    assert (qc.in_channels, qc.out_channels, qc.kernel_size) == (8, 8, (1, 1))
    assert not any(hasattr(r, "time_emb_proj") for b in enc.down_blocks for r in b.resnets)


def test_encode_returns_the_diagonal_gaussian():
    from sd_standin import AutoencoderKLEncDec
    vae = AutoencoderKLEncDec()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(1, 3, 32, 48, generator=g) * 2 - 1
    dist = vae.encode(x).latent_dist
    assert tuple(dist.mean.shape) == tuple(dist.logvar.shape) == tuple(dist.std.shape) == (1, 4, 4, 6) and dist.mean.dtype == torch.float32
    moments = vae.quant_conv(vae.encoder(x))
    assert torch.equal(dist.mean, moments[:, :4]) and torch.equal(dist.logvar, moments[:, 4:].clamp(-30, 20)) and dist.mode() is dist.mean
    assert torch.equal(dist.std, torch.exp(0.5 * dist.logvar)) and dist.logvar.min() >= -30 and dist.logvar.max() <= 20
    # sample: mean + std * randn(generator), restated; the generator moves as one randn of the mean's shape moves it
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    got = dist.sample(generator=g1)
    want = dist.mean + dist.std * torch.randn(dist.mean.shape, generator=g2)
    assert tuple(got.shape) == (1, 4, 4, 6) and torch.equal(got, want) and torch.equal(g1.get_state(), g2.get_state())
    torch.manual_seed(4)
    a = dist.sample()
    torch.manual_seed(4)
    assert torch.equal(a, dist.mean + dist.std * torch.randn(dist.mean.shape))
    # the clamp is a clamp: moments far outside come back at the limits
    vae.encoder.conv_out.weight.mul_(1e4)
    wild = vae.encode(x).latent_dist.logvar
    assert wild.min() == -30 and wild.max() == 20


def test_the_downsampler_pads_right_and_bottom_only():
    from sd_standin import AutoencoderKLEncDec
    down = AutoencoderKLEncDec().encoder.down_blocks[0].downsamplers[0]
    g = torch.Generator().manual_seed(5)
    for H, W in ((8, 8), (7, 9), (2, 2)):
        x = torch.randn(1, 128, H, W, generator=g)
        y = down(x)
        want = F.conv2d(F.pad(x, (0, 1, 0, 1)), down.conv.weight, down.conv.bias, stride=2)
        assert tuple(y.shape) == (1, 128, (H - 2) // 2 + 1, (W - 2) // 2 + 1) and torch.equal(y, want)
        symmetric = F.conv2d(x, down.conv.weight, down.conv.bias, stride=2, padding=1)[:, :, :y.shape[2], :y.shape[3]]
        assert (symmetric - y).abs().max() > 0.1 * y.abs().max()              # not the UNet's downsampler: far more than rounding apart


def test_covers_is_a_structural_check():
    from sd_standin import AutoencoderKL, AutoencoderKLEncDec, TinyVAE
    from pww_hip import vae_encode as E
    half = AutoencoderKLEncDec().to(torch.bfloat16)
    assert E.covers(half, require_device=False) and E.covers(AutoencoderKLEncDec().to(torch.float16), require_device=False)
    assert not E.covers(half)                                                   # on the CPU
    assert not E.covers(AutoencoderKLEncDec(), require_device=False)            # fp32
    assert not E.covers(AutoencoderKL().to(torch.bfloat16), require_device=False)      # no encoder of the real topology
    assert not E.covers(TinyVAE().to(torch.bfloat16), require_device=False) and not E.covers(TinyVAE())
    # one attribute off: not covered
    broken = AutoencoderKLEncDec().to(torch.bfloat16)
    broken.encoder.down_blocks[1].downsamplers[0].conv.padding = (1, 1)
    assert not E.covers(broken, require_device=False)
    broken = AutoencoderKLEncDec().to(torch.bfloat16)
    del broken.quant_conv
    assert not E.covers(broken, require_device=False)
    broken = AutoencoderKLEncDec().to(torch.bfloat16)
    broken.encoder.mid_block.attentions[0].num_heads = 8
    assert not E.covers(broken, require_device=False)
    broken = AutoencoderKLEncDec().to(torch.bfloat16)
    broken.encoder.down_blocks[0].resnets[0].time_emb_proj = nn.Linear(4, 128)
    assert not E.covers(broken, require_device=False)
    mixed = AutoencoderKLEncDec().to(torch.bfloat16)
    mixed.encoder.conv_out.float()
    assert not E.covers(mixed, require_device=False)
    mixed = AutoencoderKLEncDec().to(torch.bfloat16)
    mixed.quant_conv.to(torch.float16)
    assert not E.covers(mixed, require_device=False)
    # the decoder plug still takes the class, and the decoder's counters have the keys they had
    from pww_hip import vae as V
    assert V.covers(half, require_device=False)
    assert set(V.stats()) == {"group_norm", "conv3x3", "conv_shortcut", "upsample", "attention", "proj_attn", "tail", "decodes"}
    assert set(E.stats()) == {"head", "group_norm", "conv3x3", "conv_shortcut", "down", "attention", "proj_attn", "tail", "encodes"}


def test_the_table_row_header_and_exports(built_lib):
    import build as pww_build
    from pww_hip import _lib
    assert "vaeenc" in _lib.SIDE_EXTRA and tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA)
    spec = _lib.side_spec("vaeenc")
    assert spec is _lib.SIDE_EXTRA["vaeenc"] and set(spec) == set(_lib.SIDE["regions"]) and not spec["missing_ok"]
    assert spec["exports"] is _lib.VAEENC_EXPORTS and spec["min_version"] == _lib.VAEENC_MIN_VERSION == 100 and spec["path"] == "VAEENC_LIB_PATH"
    assert _lib.VAEENC_LIB_PATH.endswith("libpww_hip_vaeenc.so") and "PWW_HIP_VAEENC_LIB" in inspect.getsource(_lib)
    assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_vaeenc_version", "pww_vaeenc_last_error"}
    assert callable(_lib.load_vaeenc) and callable(pww_build.build_vaeenc)
    assert pww_build.SIDE_LIBS_EXTRA["vaeenc"][0] == "pww_vaeenc.hip" and pww_build.VAEENC_UNITS == [("pww_vaeenc.hip", ["-fvisibility=hidden"], "")]
    assert "pww_conv.hip" in pww_build.SIDE_LIBS_EXTRA["vaeenc"][1]             # the downsampler is that file: a change of it rebuilds this library
    assert pww_build.LIB_VAEENC == pww_build.SIDE_PATHS["vaeenc"] and "vaeenc " in pww_build.__doc__
    # the decoder's library is as it was
    assert _lib.VAE_MIN_VERSION == 100 and len(_lib.VAE_EXPORTS) == 7 and "#define PWW_VAE_VERSION 100" in open(REPO + "/include/pww_hip_vae.h").read()
    header = open(REPO + "/include/pww_hip_vaeenc.h").read()
    for line in ("#define PWW_VAEENC_VERSION 100", "#define PWW_VAEENC_IN_SAMPLE 0", "#define PWW_VAEENC_IN_UINT8 1", "#define PWW_VAEENC_HEAD_CHANNELS 128",
                 "#define PWW_VAEENC_TAIL_CHANNELS 512", "#define PWW_VAEENC_TAIL_GROUPS 32", "#define PWW_VAEENC_TAIL_MAX_CHUNKS 64"):
        assert line in header, line
    assert (_lib.VAEENC_HEAD_CHANNELS, _lib.VAEENC_TAIL_CHANNELS, _lib.VAEENC_TAIL_GROUPS, _lib.VAEENC_TAIL_MAX_CHUNKS) == (128, 512, 32, 64)
    assert (_lib.VAEENC_IN_SAMPLE, _lib.VAEENC_IN_UINT8) == (0, 1)
    for fn in spec["exports"]:
        assert "%s(" % fn in header
    source = open(PKG + "/csrc/pww_vaeenc.hip").read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_vaeenc"' in source
    assert "atomic" not in source
    # the downsampler is pww_conv.hip under a unit macro, not a second implicit GEMM
    assert "#define PWW_CONV_DOWN_UNIT 1" in source and '#include "pww_conv.hip"' in source and "PWW_CONV_DOWN_UNIT" in open(PKG + "/csrc/pww_conv.hip").read()
    entry = open(REPO + "/__graft_entry__.py").read()
    assert "for name in pww_build.SIDE_LIBS_EXTRA" in entry


def test_a_real_load_binds_the_entry_points_and_checks_arguments_on_the_host(built_lib):
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_vaeenc()
    lib = _lib.load_side("vaeenc")
    assert lib is not None and _lib.load_vaeenc() is lib and lib.pww_vaeenc_version() == 100
    for fn, (argtypes, restype) in _lib.SIDE_EXTRA["vaeenc"]["sigs"].items():
        assert getattr(lib, fn).argtypes == argtypes and getattr(lib, fn).restype is restype, fn
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.VAEENC_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in dyn.splitlines() if " T " in line and not line.split()[-1].startswith(("_init", "_fini")))
    assert visible == sorted(_lib.VAEENC_EXPORTS)          # -fvisibility=hidden: the entry points and nothing else
    # the descriptors mirror the header's structs
    assert ctypes.sizeof(_lib.VaeEncHeadDesc) == 24 and ctypes.sizeof(_lib.VaeEncDownDesc) == 36 and ctypes.sizeof(_lib.VaeEncTailDesc) == 32
    # the plan of the statistics launch is host arithmetic: chunks of whole pixels (64 where there are that many), at most 64, none empty
    sz = ctypes.sizeof(_lib.VaeEncTailDesc)
    for (B, H, W), chunks in (((1, 1, 1), 1), ((1, 8, 8), 1), ((2, 5, 7), 1), ((1, 24, 40), 15), ((2, 64, 64), 64), ((1, 64, 256), 64), ((1, 65, 63), 64)):
        d = _lib.VaeEncTailDesc(sz, _lib.DTYPE_BF16, B, H, W, 512, 1e-6, 0.18215)
        assert lib.pww_vaeenc_tail_chunks(ctypes.byref(d)) == chunks, (B, H, W)
        assert lib.pww_vaeenc_tail_workspace_bytes(ctypes.byref(d)) == B * chunks * 64 * 4 + 512 * 72 * 4
    # argument checks come before the first HIP call: they answer on a host without a device
    one = ctypes.c_void_p(16)           # (never dereferenced: every call below is refused first)
    d = _lib.VaeEncTailDesc(sz, _lib.DTYPE_BF16, 1, 8, 8, 128, 1e-6, 0.18215)
    assert lib.pww_vaeenc_tail_chunks(ctypes.byref(d)) == 0 and lib.pww_vaeenc_tail_workspace_bytes(ctypes.byref(d)) == 0 and b"512 channels" in lib.pww_last_error()
    assert lib.pww_vaeenc_tail_fwd(one, one, one, one, one, one, one, None, None, one, ctypes.byref(d), one, 1 << 20, None) == _lib.PWW_ENOTSUP
    d = _lib.VaeEncTailDesc(sz, _lib.DTYPE_BF16, 1, 8, 8, 512, 1e-6, 0.18215)
    assert lib.pww_vaeenc_tail_fwd(one, one, one, one, one, one, one, None, None, None, ctypes.byref(d), one, 1 << 20, None) == _lib.PWW_EINVAL
    assert b"required" in lib.pww_last_error()
    assert lib.pww_vaeenc_tail_fwd(None, one, one, one, one, one, one, None, None, one, ctypes.byref(d), one, 1 << 20, None) == _lib.PWW_EINVAL
    assert lib.pww_vaeenc_tail_fwd(one, one, one, one, one, one, one, None, None, one, ctypes.byref(d), one, 64, None) == _lib.PWW_EINVAL and b"workspace" in lib.pww_last_error()
    d.size = 8
    assert lib.pww_vaeenc_tail_fwd(one, one, one, one, one, one, one, None, None, one, ctypes.byref(d), one, 1 << 20, None) == _lib.PWW_EINVAL
    hd = _lib.VaeEncHeadDesc(ctypes.sizeof(_lib.VaeEncHeadDesc), _lib.DTYPE_F16, 1, 8, 8, _lib.VAEENC_IN_SAMPLE)
    assert lib.pww_vaeenc_head_fwd(None, None, one, one, one, ctypes.byref(hd), None) == _lib.PWW_EINVAL and b"required" in lib.pww_last_error()
    hd.form = _lib.VAEENC_IN_UINT8
    assert lib.pww_vaeenc_head_fwd(one, None, one, one, one, ctypes.byref(hd), None) == _lib.PWW_EINVAL and b"table" in lib.pww_last_error()
    hd.form = 2
    assert lib.pww_vaeenc_head_fwd(one, one, one, one, one, ctypes.byref(hd), None) == _lib.PWW_ENOTSUP
    hd = _lib.VaeEncHeadDesc(ctypes.sizeof(_lib.VaeEncHeadDesc), _lib.DTYPE_F16, 1, 0, 8, _lib.VAEENC_IN_SAMPLE)
    assert lib.pww_vaeenc_head_fwd(one, None, one, one, one, ctypes.byref(hd), None) == _lib.PWW_EINVAL
    dsz = ctypes.sizeof(_lib.VaeEncDownDesc)
    for args, code, text in (((1, 8, 8, 96, 128, 0, 0), _lib.PWW_ENOTSUP, b"multiples of 64"), ((1, 1, 8, 128, 128, 0, 0), _lib.PWW_ENOTSUP, b">= 2"),
                             ((1, 8, 1, 128, 128, 0, 0), _lib.PWW_ENOTSUP, b">= 2"), ((1, 8, 8, 128, 320, 160, 0), _lib.PWW_ENOTSUP, b"tile_n"),
                             ((1, 8, 8, 128, 128, 0, 99), _lib.PWW_ENOTSUP, b"split")):
        dd = _lib.VaeEncDownDesc(dsz, _lib.DTYPE_BF16, *args)
        assert lib.pww_vaeenc_down_fwd(one, one, one, one, ctypes.byref(dd), None, 0, None) == code, args
        assert text in lib.pww_last_error(), (args, lib.pww_last_error())
        assert lib.pww_vaeenc_down_workspace_bytes(ctypes.byref(dd)) == 0
    dd = _lib.VaeEncDownDesc(dsz, _lib.DTYPE_BF16, 1, 8, 8, 128, 128, 0, 0)
    assert lib.pww_vaeenc_down_fwd(None, one, one, one, ctypes.byref(dd), None, 0, None) == _lib.PWW_EINVAL and b"required" in lib.pww_last_error()
    dd.splitk = 2           # the split needs its workspace: [2][M = 16][128] fp32
    assert lib.pww_vaeenc_down_workspace_bytes(ctypes.byref(dd)) == 2 * 16 * 128 * 4
    assert lib.pww_vaeenc_down_fwd(one, one, one, one, ctypes.byref(dd), None, 0, None) == _lib.PWW_EINVAL and b"workspace" in lib.pww_last_error()


def test_a_missing_file_is_an_error(monkeypatch, tmp_path):
    import pytest
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "vaeenc", None)
    monkeypatch.setattr(_lib, "VAEENC_LIB_PATH", str(tmp_path / "libpww_hip_vaeenc.so"))
    with pytest.raises(_lib.PwwHipError, match="libpww_hip_vaeenc.so not found .*rebuild"):
        _lib.load_vaeenc()


def test_preprocess_uint8_is_what_preprocess_is_made_of():
    from PIL import Image
    from pww_hip import vae_encode as E
    pw = importlib.import_module("paint_with_words.paint_with_words")
    g = torch.Generator().manual_seed(2)
    rgb = torch.randint(0, 256, (70, 100, 3), generator=g, dtype=torch.uint8).numpy()
    rgb.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                     # every value occurs ...
    image = Image.fromarray(rgb)
    u8 = pw.preprocess_uint8(image)
    assert u8.dtype == np.uint8 and u8.shape == (1, 64, 96, 3)                  # the next lower multiple of 32
    assert np.array_equal(u8[0], np.asarray(image.resize((96, 64), resample=Image.LANCZOS)))
    want = pw.preprocess(image)
    assert tuple(want.shape) == (1, 3, 64, 96) and want.dtype == torch.float32
    exact = Image.fromarray((np.arange(32 * 32 * 3) % 256).astype(np.uint8).reshape(32, 32, 3))       # 32 x 32: no resize, all 256 values
    assert set(np.unique(pw.preprocess_uint8(exact))) == set(range(256)) and np.array_equal(pw.preprocess_uint8(exact)[0], np.asarray(exact))
    for img in (image, exact):
        pixels = torch.from_numpy(pw.preprocess_uint8(img))
        restated = 2.0 * (pixels.to(torch.float32) / 255.0) - 1.0               # 2 (u8 / 255) - 1 in fp32
        assert torch.equal(restated.permute(0, 3, 1, 2), pw.preprocess(img))    # ... and the two agree bit for bit
        for dtype in (torch.float16, torch.bfloat16):                           # the table the kernel is given holds those very values, cast
            table = E.pixel_table(dtype, "cpu")
            assert tuple(table.shape) == (256,) and table.dtype == dtype
            assert torch.equal(table[pixels.long()].permute(0, 3, 1, 2), pw.preprocess(img).to(dtype))


def test_tiny_vae_never_enters_the_plug(monkeypatch):
    """_held_images with a VAE the plug does not cover is the code of before: the plug's encode is not called, whatever the switches say."""
    import os
    from PIL import Image
    from pww_hip import vae_encode as E
    from sd_standin import AutoencoderKL, LMSDiscreteScheduler, TinyVAE
    pw = importlib.import_module("paint_with_words.paint_with_words")
    sch = LMSDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    sch.set_timesteps(4)
    g = torch.Generator().manual_seed(1)
    init = Image.fromarray(torch.randint(0, 256, (64, 64, 3), generator=g, dtype=torch.uint8).numpy())
    for vae in (TinyVAE(), AutoencoderKL()):
        tools = (vae, None, None, None, sch)
        for env in (None, "1", "0"):
            if env is None:
                monkeypatch.delenv("PWW_VAE_ENCODE", raising=False)
            else:
                monkeypatch.setenv("PWW_VAE_ENCODE", env)
            E.reset_stats()
            torch.manual_seed(7)
            lats, _, x0, noise = pw._held_images(tools, "cpu", [0], sch.timesteps, None, [init])
            st = E.stats()
            assert st["encodes"] == 0 and all(st[k] == {"native": 0, "stock": 0} for k in E._PARTS)
            # ... and is the stock code, restated
            torch.manual_seed(7)
            want = 0.18215 * vae.encode(pw.preprocess(init).to(vae.dtype)).latent_dist.sample().float()
            n = torch.randn(want.shape)
            assert torch.equal(x0, want) and torch.equal(noise, n) and torch.equal(lats, sch.add_noise(want, n, sch.timesteps[:1]))
            assert torch.equal(pw._encode_scaled(vae, pw.preprocess(init)), 0.18215 * vae.encode(pw.preprocess(init)).latent_dist.sample())
    assert E.enabled() is False and os.environ["PWW_VAE_ENCODE"] == "0"
    for name, fn in (("PWW_VAE_ENC_HEAD", E.head_enabled), ("PWW_VAE_ENC_DOWN", E.down_enabled), ("PWW_VAE_ENC_TAIL", E.tail_enabled)):
        monkeypatch.setenv(name, "0")
        assert fn() is False
        monkeypatch.setenv(name, "1")
        assert fn() is True
