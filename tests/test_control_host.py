"""ControlNet without a device: the header against the loader's table, the row order of the table pair, every refusal of
libpww_hip_control.so (in front of the first HIP runtime call, with pointers that are never dereferenced), the tile walk of the grouped
launch (pww_control_plan) over a sweep of problem sets, the stand-in's semantics on the CPU in fp32, the keywords of the public face and the
errors of the combinations that are not taken."""
import ctypes
import inspect
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import control_cases as CC
import pww_cases as cases


@pytest.fixture(scope="module")
def control_lib(built_lib):
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_side("control")
    return _lib.load_side("control")


# ---- the header, the tables, the build

def test_the_header_declares_the_exports_and_nothing_else_is_visible(control_lib):
    from pww_hip import _lib
    header = open(cases.REPO + "/include/pww_hip_control.h").read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"\b(pww_control_[a-z_]+)\s*\(", code)
    assert sorted(declared) == sorted(_lib.CONTROL_EXPORTS) and len(declared) == len(set(declared))
    assert "#define PWW_CONTROL_VERSION 100" in header and "#define PWW_CONTROL_MAX_PROBLEMS 16" in header
    assert (_lib.CONTROL_MAX_PROBLEMS, _lib.CONTROL_TILE_M, _lib.CONTROL_TILE_N) == (16, 128, 64) == (16, CC.TILE_M, CC.TILE_N)
    assert "ONE rounding" in header and "rounds three times" in header                     # the header says how the result differs from the stock one
    assert control_lib.pww_control_version() == 100 == _lib.CONTROL_MIN_VERSION
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.CONTROL_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in dyn.splitlines() if "pww_" in line.split()[-1])
    assert visible == sorted(_lib.CONTROL_EXPORTS)                                         # -fvisibility=hidden: the entry points and nothing else
    for fn, (argtypes, restype) in _lib.SIDE_EXTRA["control"]["sigs"].items():
        assert getattr(control_lib, fn).argtypes == argtypes and getattr(control_lib, fn).restype is restype, fn
    assert ctypes.sizeof(_lib.ControlProblem) == 80 and ctypes.sizeof(_lib.ControlDesc) == 16


def test_the_row_sits_in_front_of_text_in_both_tables():
    import build as pww_build
    from pww_hip import _lib
    assert tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA)
    assert tuple(_lib.SIDE_EXTRA)[-2:] == ("control", "text")
    spec = _lib.side_spec("control")
    assert spec is _lib.SIDE_EXTRA["control"] and set(spec) == set(_lib.SIDE["regions"]) and spec["missing_ok"] is True
    assert spec["exports"] is _lib.CONTROL_EXPORTS and spec["path"] == "CONTROL_LIB_PATH" and _lib.CONTROL_LIB_PATH.endswith("libpww_hip_control.so")
    assert pww_build.SIDE_LIBS_EXTRA["control"][0] == "pww_control.hip" and pww_build.CONTROL_UNITS == [("pww_control.hip", ["-fvisibility=hidden"], "")]
    assert pww_build.LIB_CONTROL == pww_build.SIDE_PATHS["control"] and callable(pww_build.build_control) and callable(_lib.load_control)
    doc = pww_build.__doc__
    assert "Fifteen libraries" in doc and doc.index("sixteenth") > doc.index("Fifteen libraries") and "control " in doc
    source = open(cases.PKG + "/csrc/pww_control.hip").read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_control"' in source
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', source)
    assert "WRITTEN AGAIN" in source and includes == ["pww_side_host.h", "../../include/pww_hip_control.h"]      # the loop is restated: no unit or header of the linear or conv kernels is included


def test_a_missing_file_declines(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "control", None)
    monkeypatch.setattr(_lib, "CONTROL_LIB_PATH", str(tmp_path / "libpww_hip_control.so"))
    assert _lib.load_control() is None                                                     # missing_ok: the stock route computes the same thing


# ---- every refusal, in front of the first HIP runtime call

P, NULL = 0x10000, None        # P is never dereferenced: validation precedes every launch
EINVAL, ENOTSUP = -22, -95


def _table(shapes, **over):
    from pww_hip import _lib
    t = (_lib.ControlProblem * max(len(shapes), 1))()
    for e, (M, N, K) in zip(t, shapes):
        e.h, e.w, e.bias, e.skip, e.out = P, P, P, P, P
        e.M, e.N, e.K = M, N, K
    for k, v in over.items():
        setattr(t[0], k, v)
    return t


def _fwd(lib, shapes, n=None, dtype=0, size=None, scale=P, index=0, **over):
    from pww_hip import _lib
    d = _lib.ControlDesc(ctypes.sizeof(_lib.ControlDesc) if size is None else size, dtype, len(shapes) if n is None else n, index)
    return lib.pww_control_fwd(_table(shapes, **over), ctypes.byref(d), ctypes.c_void_p(scale), None)


REFUSALS = [
    ("n > 16", dict(shapes=[(8, 64, 64)] * 17), EINVAL, "17 problems"),
    ("n = 0", dict(shapes=[(8, 64, 64)], n=0), EINVAL, "0 problems"),
    ("K % 64", dict(shapes=[(8, 64, 96)]), ENOTSUP, "multiples of 64"),
    ("N % 64", dict(shapes=[(8, 32, 64)]), ENOTSUP, "multiples of 64"),
    ("M = 0", dict(shapes=[(0, 64, 64)]), ENOTSUP, "M >= 1"),
    ("h stride % 8", dict(shapes=[(8, 64, 64)], h_stride=68), ENOTSUP, "multiples of 8"),
    ("skip stride % 8", dict(shapes=[(8, 64, 64)], skip_stride=100), ENOTSUP, "multiples of 8"),
    ("out stride short", dict(shapes=[(8, 64, 64)], out_stride=56), ENOTSUP, "cover their rows"),
    ("2^31", dict(shapes=[(1 << 25, 64, 64)]), ENOTSUP, "2\\^31"),
    ("h NULL", dict(shapes=[(8, 64, 64)], h=NULL), EINVAL, "are required"),
    ("w NULL", dict(shapes=[(8, 64, 64)], w=NULL), EINVAL, "are required"),
    ("bias NULL", dict(shapes=[(8, 64, 64)], bias=NULL), EINVAL, "are required"),
    ("out NULL", dict(shapes=[(8, 64, 64)], out=NULL), EINVAL, "are required"),
    ("h misaligned", dict(shapes=[(8, 64, 64)], h=P + 8), EINVAL, "16-byte aligned"),
    ("bias misaligned", dict(shapes=[(8, 64, 64)], bias=P + 4), EINVAL, "8-byte aligned"),
    ("scale NULL", dict(shapes=[(8, 64, 64)], scale=NULL), EINVAL, "scale word"),
    ("scale index", dict(shapes=[(8, 64, 64)], index=-1), EINVAL, "scale word"),
    ("size", dict(shapes=[(8, 64, 64)], size=12), EINVAL, "size 12"),
    ("size larger", dict(shapes=[(8, 64, 64)], size=24), EINVAL, "size 24"),
    ("dtype", dict(shapes=[(8, 64, 64)], dtype=2), ENOTSUP, "dtype 2"),
]


@pytest.mark.parametrize("name,kw,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_back_with_their_code_and_a_text(control_lib, name, kw, code, text):
    """No device is touched: this host has none, and a HIP call would come back as PWW_EHIP (-5)."""
    assert _fwd(control_lib, **kw) == code
    assert re.search(text, control_lib.pww_control_last_error().decode()), control_lib.pww_control_last_error()


def test_a_missing_table_or_descriptor(control_lib):
    from pww_hip import _lib
    d = _lib.ControlDesc(16, 0, 1, 0)
    assert control_lib.pww_control_fwd(None, ctypes.byref(d), ctypes.c_void_p(P), None) == EINVAL
    assert control_lib.pww_control_fwd(_table([(8, 64, 64)]), None, ctypes.c_void_p(P), None) == EINVAL
    assert control_lib.pww_control_plan(None, 1, None, 0) == EINVAL
    assert control_lib.pww_control_plan(_table([(8, 64, 64)]), 1, None, 4) == EINVAL          # room promised, none given


# ---- the tile walk

def _plan(lib, shapes):
    table = _table(shapes)
    count = lib.pww_control_plan(table, len(shapes), None, 0)
    assert count > 0
    buf = (ctypes.c_int32 * (3 * count))()
    assert lib.pww_control_plan(table, len(shapes), buf, count) == count
    return [tuple(buf[3 * t:3 * t + 3]) for t in range(count)]


@pytest.mark.parametrize("shapes", CC.PLAN_SWEEP, ids=["%dx(%d,%d,%d)" % ((len(s),) + s[0]) for s in CC.PLAN_SWEEP])
def test_every_output_tile_appears_exactly_once_in_descending_k(control_lib, shapes):
    tiles = _plan(control_lib, shapes)
    assert sorted(tiles) == sorted(CC.expected_tiles(shapes)) and len(set(tiles)) == len(tiles)
    ks = [shapes[p][2] for p, _, _ in tiles]
    assert all(a >= b for a, b in zip(ks, ks[1:]))                                         # the long K loops are issued first
    order = [p for i, (p, _, _) in enumerate(tiles) if i == 0 or tiles[i - 1][0] != p]
    assert len(order) == len(shapes)                                                       # a problem's tiles are consecutive
    assert all(shapes[a][2] > shapes[b][2] or a < b for a, b in zip(order, order[1:]))     # ties keep the caller's order


def test_the_sd15_launch_is_about_1640_tiles(control_lib):
    assert len(_plan(control_lib, CC.PLAN_SWEEP[-2])) == 3 * 64 * 5 + 16 * 5 + 2 * 16 * 10 + 4 * 10 + 2 * 4 * 20 + 4 * 20 == 1640
    assert control_lib.pww_control_plan(_table([(8, 64, 64)] * 16), 16, (ctypes.c_int32 * 6)(), 2) == 16      # a short buffer is filled, the count returned


# ---- the stand-in's semantics, on the CPU in fp32

@pytest.fixture(scope="module")
def tiny():
    from sd_standin import build_unet, build_controlnet
    unet = build_unet(CC.REQUEST_CONFIG, seed=1234)
    net = build_controlnet(CC.REQUEST_CONFIG, seed=1239)
    g = torch.Generator().manual_seed(5)
    x, ctx = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 7, 64, generator=g)
    cond = torch.rand(2, 3, 128, 128, generator=g)
    return unet, net, x, ctx, cond


def test_build_controlnet_follows_build_unet():
    from sd_standin import build_controlnet, ControlNetModel, SD15_CONFIG
    torch.manual_seed(77)
    before = torch.random.get_rng_state()
    a = build_controlnet(CC.REQUEST_CONFIG)
    assert torch.equal(torch.random.get_rng_state(), before)                               # the RNG stream did not move
    b = build_controlnet(CC.REQUEST_CONFIG)
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))
    assert isinstance(a, ControlNetModel) and not a.training and not any(p.requires_grad for p in a.parameters())
    assert len(a.controlnet_down_blocks) == 1 + 3 * 2 + 1 == 8 and all(c.kernel_size == (1, 1) for c in a.controlnet_down_blocks)
    assert float(a.controlnet_mid_block.weight.abs().max()) > 0                            # default init: a trained ControlNet's are not zero
    z = build_controlnet(CC.REQUEST_CONFIG, zero_init=True)
    assert all(float(c.weight.abs().max()) == 0 and float(c.bias.abs().max()) == 0 for c in list(z.controlnet_down_blocks) + [z.controlnet_mid_block])
    emb = a.controlnet_cond_embedding
    assert [(c.in_channels, c.out_channels, c.stride[0]) for c in [emb.conv_in] + list(emb.blocks) + [emb.conv_out]] == [
        (3, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2), (256, 64, 1)]
    with torch.device("meta"):
        sd15 = ControlNetModel(**{k: v for k, v in SD15_CONFIG.items() if k != "out_channels"})
    assert [c.in_channels for c in sd15.controlnet_down_blocks] == [320] * 4 + [640] * 3 + [1280] * 5 and sd15.controlnet_mid_block.in_channels == 1280


def test_the_none_keywords_give_the_bits_of_the_old_forward(tiny):
    unet, net, x, ctx, cond = tiny
    with torch.no_grad():
        old = unet(x, 500.0, ctx).sample
        new = unet(x, 500.0, ctx, down_block_additional_residuals=None, mid_block_additional_residual=None).sample
    assert torch.equal(old, new)
    params = inspect.signature(type(unet).forward).parameters
    assert list(params)[-2:] == ["down_block_additional_residuals", "mid_block_additional_residual"] and all(params[k].default is None for k in list(params)[-2:])


def test_the_residuals_match_the_skips_and_steer_the_unet(tiny):
    unet, net, x, ctx, cond = tiny
    with torch.no_grad():
        down, mid = net(x, 500.0, ctx, cond, conditioning_scale=1.0)
        # the skips of the UNet: conv_in's output and every output of the down blocks
        temb_shapes = [(2, 64, 16, 16), (2, 64, 16, 16), (2, 64, 8, 8), (2, 128, 8, 8), (2, 128, 4, 4), (2, 128, 4, 4), (2, 128, 2, 2), (2, 128, 2, 2)]
        assert [tuple(d.shape) for d in down] == temb_shapes and tuple(mid.shape) == (2, 128, 2, 2)
        plain = unet(x, 500.0, ctx).sample
        steered = unet(x, 500.0, ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
        half_down, half_mid = net(x, 500.0, ctx, cond, conditioning_scale=0.5)
    assert not torch.equal(plain, steered) and float((plain - steered).abs().max()) > 1e-4
    assert all(torch.equal(h, 0.5 * d) for h, d in zip(half_down, down)) and torch.equal(half_mid, 0.5 * mid)
    with torch.no_grad():
        other, _ = net(x, 500.0, ctx, 1.0 - cond)
    assert not torch.equal(other[0], down[0])                                              # the control image matters


def test_zeroed_zero_convolutions_or_scale_zero_give_the_uncontrolled_bits(tiny):
    from sd_standin import build_controlnet
    unet, net, x, ctx, cond = tiny
    with torch.no_grad():
        plain = unet(x, 500.0, ctx).sample
        down, mid = net(x, 500.0, ctx, cond, conditioning_scale=0.0)
        assert torch.equal(unet(x, 500.0, ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample, plain)
        zeroed = build_controlnet(CC.REQUEST_CONFIG, zero_init=True)
        down, mid = zeroed(x, 500.0, ctx, cond, conditioning_scale=1.0)
        assert all(float(d.abs().max()) == 0 for d in down) and float(mid.abs().max()) == 0
        assert torch.equal(unet(x, 500.0, ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample, plain)


# ---- covers, the request object, the guidance window

def test_covers_decides_by_layout():
    from pww_hip import controlnet as CN
    from sd_standin import build_controlnet, build_unet
    net = build_controlnet(CC.REQUEST_CONFIG, dtype=torch.float16)
    assert CN.covers(net, require_device=False) and not CN.covers(net)                      # on the CPU: the layout, but no device
    assert not CN.covers(build_controlnet(CC.REQUEST_CONFIG), require_device=False)         # fp32
    assert not CN.covers(build_unet(CC.REQUEST_CONFIG, dtype=torch.float16), require_device=False)      # a UNet has no zero convolutions
    odd = build_controlnet(CC.REQUEST_CONFIG, dtype=torch.float16)
    odd.controlnet_mid_block = torch.nn.Conv2d(128, 128, 3, padding=1).half()
    assert not CN.covers(odd, require_device=False)
    doc = open(cases.REPO + "/INTEGRATION.md").read()
    assert "covered by layout only" in doc


def test_the_request_and_its_window():
    from pww_hip import controlnet as CN
    from sd_standin import build_controlnet
    net = build_controlnet(CC.REQUEST_CONFIG, dtype=torch.float16)
    im = torch.zeros(1, 3, 128, 128)
    r = CN.ControlRequest([net], [im], [0.8], 0.0, 0.5)
    assert [r.active(i, 3) for i in range(3)] == [True, False, False] and r.words(0, 3) == [0.8] and r.words(1, 3) == [0.0]
    assert [r.active(i, 30) for i in range(30)] == [True] * 15 + [False] * 15
    full = CN.ControlRequest([net, net], [im, im], [1.0, 0.25])
    assert all(full.active(i, 7) for i in range(7)) and full.words(3, 7) == [1.0, 0.25]
    for s, e in ((0.0, 0.0), (0.5, 0.5), (1.0, 1.0)):                                       # start == end: no step is inside
        empty = CN.ControlRequest([net], [im], [1.0], s, e)
        assert not any(empty.active(i, 3) for i in range(3)) and not any(empty.active(i, 30) for i in range(30))
    for bad in (dict(nets=[], images=[], scales=[]), dict(nets=[net] * 5, images=[im] * 5, scales=[1.0] * 5), dict(nets=[net], images=[im, im], scales=[1.0]),
                dict(nets=[net], images=[im], scales=[1.0], start=0.6, end=0.4), dict(nets=[net], images=[im], scales=[1.0], end=1.5),
                dict(nets=[net], images=[im], scales=[float("nan")]), dict(nets=[net], images=[im[0]], scales=[1.0]),
                dict(nets=[torch.nn.Conv2d(3, 3, 1)], images=[im], scales=[1.0])):
        with pytest.raises(ValueError, match="controlnet"):
            CN.ControlRequest(**bad)
    assert CN.mode() in ("0", "1", "force") and set(CN.stats()) >= {"grouped_launches", "stock_zero_convs", "declined", "decline_reasons", "hint_embeddings"}


def test_pww_control_must_be_a_known_value(monkeypatch):
    from pww_hip import controlnet as CN
    for v in ("0", "1", "force"):
        monkeypatch.setenv("PWW_CONTROL", v)
        assert CN.mode() == v
    monkeypatch.setenv("PWW_CONTROL", "yes")
    with pytest.raises(ValueError, match="PWW_CONTROL"):
        CN.mode()
    monkeypatch.delenv("PWW_CONTROL")
    assert CN.mode() == CN.DEFAULT


# ---- the public face: the keywords, the control image, the combinations that are not taken

def test_keywords_and_their_defaults():
    import paint_with_words as pw
    names5 = ["controlnet", "control_image", "controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end"]
    for f in (pw.paint_with_words, pw.paint_with_words_batch):
        params = inspect.signature(f).parameters
        names = list(params)
        at = names.index("controlnet")
        assert names[at:at + 5] == names5 and at > names.index("strength") and names[-1] == "max_prompt_chunks"
        assert [params[k].default for k in names5] == [None, None, 1.0, 0.0, 1.0]
        assert "controlnet" in f.__doc__ and "control_image" in f.__doc__
    from pww_hip.sampler import PwWSampler
    assert inspect.signature(PwWSampler.sample).parameters["control"].default is None


def test_control_images_of_every_kind_and_their_errors():
    from paint_with_words.paint_with_words import _control_image_tensor, _control_request
    from sd_standin import build_controlnet
    rgb = CC.control_image(1)
    a = _control_image_tensor(Image.fromarray(rgb), (128, 128))
    b = _control_image_tensor(rgb, (128, 128))
    c = _control_image_tensor(torch.from_numpy(rgb).permute(2, 0, 1).float() / 255.0, (128, 128))
    assert a.dtype == torch.float32 and tuple(a.shape) == (3, 128, 128) and torch.equal(a, b) and torch.equal(a, c) and 0 <= float(a.min()) and float(a.max()) <= 1
    gray = _control_image_tensor(rgb[:, :, 0], (128, 128))
    assert torch.equal(gray[0], a[0]) and torch.equal(gray[1], a[0])
    for bad, match in ((rgb[:64], "same size"), (Image.fromarray(rgb).resize((64, 128)), "same size"), (rgb.astype(np.float32), "uint8"), ("x.png", "PIL image"),
                       (torch.zeros(3, 128, 128, dtype=torch.uint8), "float"), (torch.full((3, 128, 128), 2.0), r"\[0, 1\]"), (torch.zeros(3, 64, 128), "same size")):
        with pytest.raises(ValueError, match=match):
            _control_image_tensor(bad, (128, 128))
    net = build_controlnet(CC.REQUEST_CONFIG, dtype=torch.float16)
    assert _control_request(None, None, 1.0, 0.0, 1.0, 1, (128, 128)) is None
    r = _control_request(net, rgb, 0.7, 0.1, 0.9, 3, (128, 128))
    assert r.nets == [net] and tuple(r.images[0].shape) == (3, 3, 128, 128) and r.scales == [0.7] and (r.start, r.end) == (0.1, 0.9)
    other = CC.control_image(2)
    r = _control_request([net, net], [rgb, [rgb, other]], [1.0, 0.5], 0.0, 1.0, 2, (128, 128))
    assert len(r.images) == 2 and torch.equal(r.images[1][0], a) and not torch.equal(r.images[1][1], a) and r.scales == [1.0, 0.5]
    for args, match in (((None, rgb, 1.0, 0.0, 1.0, 1), "without a controlnet"), ((net, None, 1.0, 0.0, 1.0, 1), "needs a control_image"),
                        (([net] * 5, [rgb] * 5, 1.0, 0.0, 1.0, 1), "1 .. 4"), (([net, net], rgb, 1.0, 0.0, 1.0, 1), "list of 2 control images"),
                        ((net, [rgb, rgb], 1.0, 0.0, 1.0, 3), "2 entries for 3 requests"), ((net, rgb, [1.0, 2.0], 0.0, 1.0, 1), "conditioning_scale"),
                        ((net, rgb, "1", 0.0, 1.0, 1), "conditioning_scale"), ((net, rgb, 1.0, None, 1.0, 1), "control_guidance"),
                        ((net, rgb, 1.0, 0.5, 0.25, 1), "control_guidance_start")):
        with pytest.raises(ValueError, match=match):
            _control_request(*args, (128, 128))


def test_the_combinations_that_are_not_taken_say_so():
    import importlib
    import paint_with_words as pw
    from paint_with_words import pipelines
    from pww_hip import dist
    from sd_standin import build_controlnet
    net = build_controlnet(CC.REQUEST_CONFIG, dtype=torch.float16)
    rgb, cmap = CC.control_image(1), Image.fromarray(CC.color_map())
    with pytest.raises(ValueError, match="canvas_window"):
        pw.paint_with_words(dict(cases.RUNNER_CONTEXT), cmap, cases.RUNNER_PROMPT, controlnet=net, control_image=rgb, canvas_window=64)
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    for f, args in ((inp.paint_with_words_inpaint, ()), (inp.paint_with_words_inpaint_batch, ({}, cmap, cmap, cmap, "", [0]))):
        assert "controlnet" in inspect.signature(f).parameters
        with pytest.raises(ValueError, match="inpaint functions"):
            f(*args, controlnet=net, control_image=rgb)
    for cls in (pipelines.PaintWithWord_StableDiffusionPipeline, pipelines.PaintWithWord_StableDiffusionInpaintPipeline):
        assert cls.controlnet is None and "controlnet" not in inspect.signature(cls.__call__).parameters
        pipe = cls.__new__(cls)
        pipe.controlnet = net
        with pytest.raises(ValueError, match="pipeline classes"):
            pipe._check_extensions()
    with pytest.raises(ValueError, match="pww_hip.dist"):
        dist.broadcast_request({"rgb": rgb, "controlnet": net}, "cpu")
    assert dist.broadcast_request({"rgb": rgb}, "cpu")["rgb"] is rgb                         # (a request without one passes through as before)
