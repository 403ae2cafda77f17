"""Host side of the AutoencoderKL decode: the stand-in's layout, the plug's structural check, the side library's table rows, and that a VAE
the plug does not cover never enters it. No GPU."""
import inspect
import os
import subprocess

import numpy as np
import torch
import torch.nn as nn

from conftest import PKG, REPO


def test_autoencoder_kl_has_the_diffusers_layout_and_decodes():
    from sd_standin import AutoencoderKL, TinyVAE
    vae = AutoencoderKL()
    dec = vae.decoder
    assert isinstance(vae.post_quant_conv, nn.Conv2d) and vae.post_quant_conv.kernel_size == (1, 1) and vae.post_quant_conv.out_channels == 4
    assert dec.conv_in.in_channels == 4 and dec.conv_in.out_channels == 512 and dec.conv_in.kernel_size == (3, 3)
    mid = dec.mid_block
    assert len(mid.resnets) == 2 and len(mid.attentions) == 1
    a = mid.attentions[0]
    for n in ("query", "key", "value", "proj_attn"):
        assert isinstance(getattr(a, n), nn.Linear) and getattr(a, n).weight.shape == (512, 512)
    assert a.group_norm.num_groups == 32 and a.num_heads == 1 and a.channels == 512
    assert [b.resnets[-1].conv2.out_channels for b in dec.up_blocks] == [512, 512, 256, 128]
    assert [len(b.resnets) for b in dec.up_blocks] == [3, 3, 3, 3]
    assert [b.upsamplers is not None for b in dec.up_blocks] == [True, True, True, False]
    assert [b.resnets[0].conv_shortcut is not None for b in dec.up_blocks] == [False, False, True, True]
    assert all(r.conv_shortcut is None for b in dec.up_blocks for r in b.resnets[1:])
    assert dec.up_blocks[2].resnets[0].conv_shortcut.kernel_size == (1, 1) and not hasattr(mid.resnets[0], "time_emb_proj")
    norms = [m for m in vae.modules() if isinstance(m, nn.GroupNorm)]
    assert len(norms) == 2 * 14 + 2 and all(m.num_groups == 32 and m.eps == 1e-6 for m in norms)
    assert dec.conv_norm_out.num_channels == 128 and dec.conv_out.out_channels == 3 and dec.conv_out.in_channels == 128
    # seeded: the same weights twice, and the global generator untouched
    state = torch.random.get_rng_state()
    again = AutoencoderKL()
    assert torch.equal(torch.random.get_rng_state(), state)
    assert all(torch.equal(p, q) for p, q in zip(vae.parameters(), again.parameters()))
    g = torch.Generator().manual_seed(3)
    out = vae.decode(torch.randn(1, 4, 4, 6, generator=g))
    assert tuple(out.sample.shape) == (1, 3, 32, 48) and out.sample.dtype == torch.float32 and torch.isfinite(out.sample).all()
    # encode is TinyVAE's stand-in, so img2img runs on the class
    lat = vae.encode(torch.zeros(1, 3, 32, 48)).latent_dist.sample()
    assert tuple(lat.shape) == (1, 4, 4, 6) and "encode" in AutoencoderKL.__doc__
    assert isinstance(TinyVAE().dec, nn.Conv2d)


def test_covers_is_a_structural_check():
    from sd_standin import AutoencoderKL, TinyVAE
    from pww_hip import vae as V
    half = AutoencoderKL().to(torch.bfloat16)
    assert V.covers(half, require_device=False) and V.covers(AutoencoderKL().to(torch.float16), require_device=False)
    assert not V.covers(half)                                            # on the CPU
    assert not V.covers(AutoencoderKL(), require_device=False)           # fp32
    assert not V.covers(TinyVAE().to(torch.bfloat16), require_device=False) and not V.covers(TinyVAE())
    # one attribute off: not covered
    broken = AutoencoderKL().to(torch.bfloat16)
    broken.decoder.mid_block.attentions[0].num_heads = 8
    assert not V.covers(broken, require_device=False)
    broken = AutoencoderKL().to(torch.bfloat16)
    del broken.decoder.conv_norm_out
    assert not V.covers(broken, require_device=False)
    mixed = AutoencoderKL().to(torch.bfloat16)
    mixed.decoder.conv_out.float()
    assert not V.covers(mixed, require_device=False)


def test_the_table_row_header_and_exports(built_lib):
    import build as pww_build
    from pww_hip import _lib
    assert "vae" in _lib.SIDE_EXTRA and tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA)
    spec = _lib.side_spec("vae")
    assert spec is _lib.SIDE_EXTRA["vae"] and set(spec) == set(_lib.SIDE["regions"]) and not spec["missing_ok"]
    assert spec["exports"] is _lib.VAE_EXPORTS and spec["min_version"] == _lib.VAE_MIN_VERSION == 100 and spec["path"] == "VAE_LIB_PATH"
    assert _lib.VAE_LIB_PATH.endswith("libpww_hip_vae.so") and "PWW_HIP_VAE_LIB" in inspect.getsource(_lib)
    assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_vae_version", "pww_vae_last_error"}
    assert pww_build.SIDE_LIBS_EXTRA["vae"][0] == "pww_vae.hip" and pww_build.VAE_UNITS == [("pww_vae.hip", ["-fvisibility=hidden"], "")]
    assert pww_build.LIB_VAE == pww_build.SIDE_PATHS["vae"] and "vae " in pww_build.__doc__
    header = open(REPO + "/include/pww_hip_vae.h").read()
    assert "#define PWW_VAE_VERSION 100" in header and "#define PWW_VAE_HEAD_DIM 512" in header and "#define PWW_VAE_TAIL_CHANNELS 128" in header
    assert (_lib.VAE_HEAD_DIM, _lib.VAE_TAIL_CHANNELS, _lib.VAE_TAIL_GROUPS, _lib.VAE_TAIL_MAX_CHUNKS) == (512, 128, 32, 64)
    assert "#define PWW_VAE_TAIL_GROUPS 32" in header and "#define PWW_VAE_TAIL_MAX_CHUNKS 64" in header
    assert "#define PWW_VAE_OUT_SAMPLE 0" in header and "#define PWW_VAE_OUT_UINT8 1" in header and (_lib.VAE_OUT_SAMPLE, _lib.VAE_OUT_UINT8) == (0, 1)
    for fn in spec["exports"]:
        assert "%s(" % fn in header
    source = open(PKG + "/csrc/pww_vae.hip").read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_vae"' in source
    assert "atomic" not in source
    entry = open(REPO + "/__graft_entry__.py").read()
    assert "for name in pww_build.SIDE_LIBS_EXTRA" in entry


def test_a_real_load_binds_the_entry_points_and_checks_arguments_on_the_host(built_lib):
    import ctypes
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_vae()
    lib = _lib.load_side("vae")
    assert lib is not None and _lib.load_vae() is lib and lib.pww_vae_version() == 100
    for fn, (argtypes, restype) in _lib.SIDE_EXTRA["vae"]["sigs"].items():
        assert getattr(lib, fn).argtypes == argtypes and getattr(lib, fn).restype is restype, fn
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.VAE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in dyn.splitlines() if " T " in line and not line.split()[-1].startswith(("_init", "_fini")))
    assert visible == sorted(_lib.VAE_EXPORTS)          # -fvisibility=hidden: the entry points and nothing else
    # the descriptors mirror the header's structs
    assert ctypes.sizeof(_lib.VaeAttnDesc) == 24 + 8 * 8 and ctypes.sizeof(_lib.VaeTailDesc) == 32
    # the plan of the statistics launch is host arithmetic: chunks of whole pixels, at most 64, none empty
    for (B, H, W), chunks in (((1, 1, 1), 1), ((1, 8, 8), 1), ((1, 24, 40), 4), ((2, 64, 64), 16), ((1, 512, 512), 64), ((1, 512, 2048), 64), ((1, 129, 127), 64)):
        d = _lib.VaeTailDesc(ctypes.sizeof(_lib.VaeTailDesc), _lib.DTYPE_BF16, B, H, W, 128, 0, 1e-6)
        assert lib.pww_vae_tail_chunks(ctypes.byref(d)) == chunks, (B, H, W)
        assert lib.pww_vae_tail_workspace_bytes(ctypes.byref(d)) == B * chunks * 64 * 4 + 128 * 28 * 4
    d = _lib.VaeTailDesc(ctypes.sizeof(_lib.VaeTailDesc), _lib.DTYPE_BF16, 1, 8, 8, 64, 0, 1e-6)
    assert lib.pww_vae_tail_chunks(ctypes.byref(d)) == 0 and lib.pww_vae_tail_workspace_bytes(ctypes.byref(d)) == 0 and b"128 channels" in lib.pww_last_error()
    # argument checks come before the first HIP call: they answer on a host without a device
    d = _lib.VaeAttnDesc(ctypes.sizeof(_lib.VaeAttnDesc), _lib.DTYPE_F16, 1, 8, 512, 0.0, 4096, 512, 4096, 512, 4096, 512, 4096, 512)
    assert lib.pww_vae_attn_fwd(None, None, None, None, ctypes.byref(d), None) == _lib.PWW_EINVAL and b"required" in lib.pww_last_error()


def test_a_missing_file_is_an_error(monkeypatch, tmp_path):
    import pytest
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "vae", None)
    monkeypatch.setattr(_lib, "VAE_LIB_PATH", str(tmp_path / "libpww_hip_vae.so"))
    with pytest.raises(_lib.PwwHipError, match="libpww_hip_vae.so not found .*rebuild"):
        _lib.load_vae()


def test_tiny_vae_never_enters_the_plug(monkeypatch):
    """_pil_from_latents with a VAE the plug does not cover is the code of before: the plug's decode is not called, whatever the switches say."""
    import importlib
    pw = importlib.import_module("paint_with_words.paint_with_words")       # (the package exports a function of the same name)
    from pww_hip import vae as V
    from sd_standin import TinyVAE
    from PIL import Image
    vae = TinyVAE()
    g = torch.Generator().manual_seed(1)
    latents = torch.randn(2, 4, 4, 6, generator=g)
    for env in (None, "1", "0"):
        if env is None:
            monkeypatch.delenv("PWW_VAE", raising=False)
        else:
            monkeypatch.setenv("PWW_VAE", env)
        V.reset_stats()
        images = pw._pil_from_latents(vae, latents)
        pixels = pw._pil_from_latents(vae, latents, "np")
        st = V.stats()
        assert st["decodes"] == 0 and all(st[k] == {"native": 0, "stock": 0} for k in V._PARTS)
        # ... and is the stock code, restated
        decoded = vae.decode((latents.clone() / 0.18215).to(vae.dtype)).sample
        want = (decoded / 2 + 0.5).clamp(0, 1).detach().float().cpu().permute(0, 2, 3, 1).numpy()
        assert np.array_equal(pixels, want) and len(images) == 2 and isinstance(images[0], Image.Image)
        assert all(np.array_equal(np.asarray(im), (w * 255).round().astype("uint8")) for im, w in zip(images, want))
    assert V.enabled() is False and os.environ["PWW_VAE"] == "0"
    # the two kernel switches: the tail on, the attention off by default (measured slower than the stock sequence: profiles/vae_decode.md)
    monkeypatch.delenv("PWW_VAE_ATTN", raising=False)
    monkeypatch.delenv("PWW_VAE_TAIL", raising=False)
    assert (V.attn_enabled(), V.tail_enabled()) == (False, True)
    monkeypatch.setenv("PWW_VAE_ATTN", "1")
    monkeypatch.setenv("PWW_VAE_TAIL", "0")
    assert (V.attn_enabled(), V.tail_enabled()) == (True, False)
