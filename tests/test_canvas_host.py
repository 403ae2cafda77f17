"""Canvases larger than the UNet's window, without a device: the window grid, the table pair of the open-ended side libraries and the load of
libpww_hip_canvas.so, every argument check of its two entry points (in front of the first HIP runtime call, with pointers that are never
dereferenced), the `canvas_*` keywords of paint_with_words, what a canvas request hands to the conditioning layer and to the sampler, and
the recorded oracle loops of tests/golden/canvas_oracle.npz against fresh CPU runs."""
import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import canvas_cases as C
import pww_cases as cases
import region_prompt_cases as R
from gpu_util import rel_l2
from host_standins import cpu_masks  # noqa: F401  (fixture)
from test_entry_points_host import rig, _tools, _color_map, CONTEXT, STRIPPED, NEG, NEG_STRIPPED, PROMPT, SIDE  # noqa: F401  (rig: fixture)


# ---- the window grid

def test_canvas_windows():
    from pww_hip import ops
    assert ops.canvas_windows(20, 8, 4) == (0, 4, 8, 12)
    assert ops.canvas_windows(11, 8, 4) == (0, 3)
    assert ops.canvas_windows(8, 8, 4) == (0,)
    assert ops.canvas_windows(256, 64, 32) == (0, 32, 64, 96, 128, 160, 192)
    assert ops.canvas_windows(21, 8, 8) == (0, 8, 13)                    # stride = window: no overlap but at the clamped end
    for L, win, stride in [(20, 8, 4), (11, 8, 4), (8, 8, 4), (256, 64, 32), (97, 16, 5), (128, 128, 1), (130, 128, 64)]:
        got = ops.canvas_windows(L, win, stride)
        assert list(got) == C.windows(L, win, stride) and all(isinstance(v, int) for v in got)
        assert got[0] == 0 and got[-1] == L - win and all(0 < b - a <= stride for a, b in zip(got, got[1:]))
    for bad in [(7, 8, 4), (20, 8, 0), (20, 8, 9), (20, 0, 1)]:
        with pytest.raises(ValueError, match="canvas_windows"):
            ops.canvas_windows(*bad)


def test_canvas_plan():
    from pww_hip.sampler import canvas_plan
    assert canvas_plan((12, 11), 8, 4, 3) == {"size": (12, 11), "window": (8, 8), "ys": (0, 4), "xs": (0, 3), "ramp": 3}


# ---- the table pair, the build and the load

def test_the_open_ended_table_pair_holds_the_library(built_lib):
    import build as pww_build
    from pww_hip import _lib
    assert tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA) and "canvas" in _lib.SIDE_EXTRA
    assert not set(pww_build.SIDE_LIBS_EXTRA) & (set(pww_build.SIDE_LIBS) | set(pww_build.SIDE_LIBS_CONV))
    assert set(pww_build.SIDE_LIBS_EXTRA) <= set(pww_build.ALL_SIDE_LIBS) and set(pww_build.ALL_SIDE_LIBS) == set(pww_build.SIDE_PATHS)
    for name in _lib.SIDE_EXTRA:          # every row, whatever comes later: the fields of the other tables, found by side_spec
        spec, up = _lib.side_spec(name), name.upper()
        assert spec is _lib.SIDE_EXTRA[name] and set(spec) == set(_lib.SIDE["regions"])
        assert spec["exports"] is getattr(_lib, up + "_EXPORTS") and spec["min_version"] == getattr(_lib, up + "_MIN_VERSION")
        assert spec["path"] == up + "_LIB_PATH" and getattr(_lib, spec["path"]).endswith("libpww_hip_%s.so" % name)
        assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_%s_version" % name, "pww_%s_last_error" % name}
        assert callable(getattr(_lib, "load_" + name)) and callable(getattr(pww_build, "build_" + name))
        assert pww_build.SIDE_LIBS_EXTRA[name][0] == "pww_%s.hip" % name and "-fvisibility=hidden" in pww_build.SIDE_UNITS[name][0][1]
    spec = _lib.SIDE_EXTRA["canvas"]
    assert spec["exports"] == ("pww_canvas_version", "pww_canvas_last_error", "pww_canvas_gather", "pww_canvas_combine") and not spec["missing_ok"]
    assert pww_build.PER_FILE_FLAGS["pww_canvas.hip"] == ["-ffp-contract=off"] and pww_build.LIB_CANVAS == pww_build.SIDE_PATHS["canvas"]
    entry = open(cases.REPO + "/__graft_entry__.py").read()
    assert "for name in pww_build.SIDE_LIBS_EXTRA" in entry
    main = inspect.getsource(pww_build).split('if __name__ == "__main__":')[1]
    assert "for name in ALL_SIDE_LIBS" in main
    header = open(cases.REPO + "/include/pww_hip_canvas.h").read()
    assert "#define PWW_CANVAS_VERSION 100" in header and "#define PWW_CANVAS_MAX_WINDOWS 64" in header and "#define PWW_CANVAS_MAX_RAMP 64" in header
    assert (_lib.CANVAS_MAX_WINDOWS, _lib.CANVAS_MAX_RAMP, _lib.CANVAS_MIN_WINDOW, _lib.CANVAS_MAX_WINDOW) == (64, 64, 8, 128)
    for fn in spec["exports"]:
        assert "%s(" % fn in header
    source = open(cases.PKG + "/csrc/pww_canvas.hip").read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_canvas"' in source
    assert "atomic" not in source.replace("No atomics", "")


@pytest.fixture(scope="module")
def canvas_lib(built_lib):
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_side("canvas")
    return _lib.load_side("canvas")


def test_a_real_load_binds_the_entry_points(canvas_lib):
    from pww_hip import _lib
    assert canvas_lib is not None and _lib.load_canvas() is canvas_lib and _lib.load_side("canvas") is canvas_lib
    assert canvas_lib.pww_canvas_version() == 100
    for fn, (argtypes, restype) in _lib.SIDE_EXTRA["canvas"]["sigs"].items():
        assert getattr(canvas_lib, fn).argtypes == argtypes and getattr(canvas_lib, fn).restype is restype, fn
    import subprocess
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.CANVAS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in dyn.splitlines() if " T " in line and not line.split()[-1].startswith(("_init", "_fini")))
    assert visible == sorted(_lib.CANVAS_EXPORTS)          # -fvisibility=hidden: the entry points and nothing else


def test_a_missing_file_is_an_error(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "canvas", None)
    monkeypatch.setattr(_lib, "CANVAS_LIB_PATH", str(tmp_path / "libpww_hip_canvas.so"))
    with pytest.raises(_lib.PwwHipError, match="libpww_hip_canvas.so not found .*rebuild"):
        _lib.load_canvas()


# ---- every PWW_EINVAL / PWW_ENOTSUP of the two entry points, in front of the first HIP runtime call

P, NULL = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)        # P is never dereferenced: validation precedes every launch
F16, BF16 = 0, 1


def _origins(values):
    return None if values is None else (ctypes.c_int32 * len(values))(*values)


def _gather(lib, canvas=P, out=P, ys=(0,), xs=(0, 4, 8, 12), ny=None, nx=None, C=4, Hc=8, Wc=20, h=8, w=8, denom=1.0, copies=1, dtype=F16):
    return lib.pww_canvas_gather(canvas, out, _origins(ys), len(ys) if ny is None else ny, _origins(xs), len(xs) if nx is None else nx, C, Hc, Wc, h, w,
                                 denom, copies, dtype, None)


def _combine(lib, eps=P, masks=NULL, weights=NULL, scales=NULL, g=7.5, out=P, ys=(0,), xs=(0, 4, 8, 12), ny=None, nx=None, K=0, C=4, Hc=8, Wc=20,
             h=8, w=8, ramp=0, dtype=F16):
    return lib.pww_canvas_combine(eps, masks, weights, scales, g, out, _origins(ys), len(ys) if ny is None else ny, _origins(xs),
                                  len(xs) if nx is None else nx, K, C, Hc, Wc, h, w, ramp, dtype, None)


EINVAL, ENOTSUP = -22, -95
# (keyword arguments, return code, a word of the error text): the cases both entry points share ...
SHARED = [
    (dict(out=NULL), EINVAL, "null"),
    (dict(ys=None, ny=1), EINVAL, "null"),
    (dict(xs=None, nx=4), EINVAL, "null"),
    (dict(xs=(0, 8, 4, 12)), EINVAL, "ascending"),                         # unsorted origins
    (dict(xs=(0, 4, 4, 12)), EINVAL, "ascending"),
    (dict(xs=(1, 4, 8, 12)), EINVAL, "first origin"),                      # first origin != 0
    (dict(xs=(0, 4, 8, 11)), EINVAL, "last origin"),                       # last origin != L - win
    (dict(xs=(0, 4, 8, 13)), EINVAL, "last origin"),                       # ... past the end
    (dict(xs=(0, 9, 12)), EINVAL, "gap"),                                  # a gap: pixel 8 is in no window
    (dict(ys=(0, 1), Hc=8), EINVAL, "last origin"),
    (dict(ys=tuple(range(5)), xs=tuple(range(13)), Hc=12, Wc=20), EINVAL, "5 x 13 windows"),       # 65 windows
    (dict(xs=tuple(range(65)), Wc=72), EINVAL, "1 x 65 windows"),
    (dict(ys=(), ny=0), EINVAL, "windows"),
    (dict(h=4, Hc=4), EINVAL, "window 4 x 8"),                             # h = 4
    (dict(w=136, xs=(0,), Wc=136), EINVAL, "window 8 x 136"),
    (dict(Hc=7), EINVAL, "smaller than the window"),
    (dict(C=0), EINVAL, "channels"),
    (dict(dtype=2), ENOTSUP, "dtype"),                                     # a bad dtype
    (dict(dtype=-1), ENOTSUP, "dtype"),
]
# ... and the ones of each
GATHER_ONLY = [(dict(canvas=NULL), EINVAL, "null"), (dict(copies=0), EINVAL, "copies"), (dict(copies=11), EINVAL, "copies"),
               (dict(denom=0.0), EINVAL, "denom"), (dict(denom=float("nan")), EINVAL, "denom"), (dict(denom=float("inf")), EINVAL, "denom")]
COMBINE_ONLY = [(dict(eps=NULL), EINVAL, "null"), (dict(K=1), EINVAL, "null"), (dict(K=1, masks=P, weights=P), EINVAL, "null"),
                (dict(K=9, masks=P, weights=P, scales=P), EINVAL, "regions"), (dict(K=-1), EINVAL, "regions"),
                (dict(ramp=65), EINVAL, "ramp"), (dict(ramp=-1), EINVAL, "ramp")]               # ramp 65


@pytest.mark.parametrize("entry", ["gather", "combine"])
def test_every_refusal_returns_before_a_hip_call_and_fills_the_error_slot(canvas_lib, entry):
    from pww_hip import _lib
    call, own = (_gather, GATHER_ONLY) if entry == "gather" else (_combine, COMBINE_ONLY)
    product = _lib.load()
    before = product.pww_last_error()
    seen = set()
    for kw, want, word in SHARED + own:
        rc = call(canvas_lib, **kw)
        text = canvas_lib.pww_canvas_last_error().decode()
        assert rc == want, (kw, rc, text)
        assert text.startswith("canvas_%s: " % entry) and word in text, (kw, text)
        seen.add(text)
        with pytest.raises(_lib.PwwHipError) as e:
            _lib.check(rc, "pww_canvas_" + entry, canvas_lib)
        assert text in str(e.value) and "rc=%d" % want in str(e.value)
    assert len(seen) >= 14                                   # each check has its own sentence
    assert product.pww_last_error() == before               # the product library's slot is another one


def test_ops_argument_checks():
    """In the style of region_combine: a CPU tensor, a wrong type or shapes that do not go together raise before the library is asked."""
    from pww_hip import ops
    from pww_hip._lib import PwwHipError
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.canvas_gather(torch.zeros(4, 8, 20), (0,), (0, 4, 8, 12), 8, 8, 1.0, 1, torch.float16)
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.canvas_combine(torch.zeros(8, 4, 8, 8, dtype=torch.float16), (0,), (0, 4, 8, 12), (8, 20), 7.5)


# ---- the public face

def _wide_map(H=64, W=160):
    return Image.fromarray(C.color_map(H, W))


BAD = [(dict(canvas_window=100), (160, 64), "canvas_window must be a multiple of 64"),
       (dict(canvas_window=0), (160, 64), "canvas_window"),
       (dict(canvas_window=1088), (2048, 1088), "canvas_window"),
       (dict(canvas_window=64.0), (160, 64), "canvas_window"),
       (dict(canvas_window=True), (160, 64), "canvas_window"),
       (dict(canvas_window=64, canvas_stride=12), (160, 64), "canvas_stride must be a multiple of 8"),
       (dict(canvas_window=64, canvas_stride=0), (160, 64), "canvas_stride"),
       (dict(canvas_window=64, canvas_stride=72), (160, 64), "canvas_stride"),
       (dict(canvas_window=64, canvas_stride=32.0), (160, 64), "canvas_stride"),
       (dict(canvas_window=64, canvas_ramp=65), (160, 64), "canvas_ramp"),
       (dict(canvas_window=64, canvas_ramp=-1), (160, 64), "canvas_ramp"),
       (dict(canvas_window=64, canvas_ramp=1.5), (160, 64), "canvas_ramp"),
       (dict(canvas_window=128), (160, 64), "smaller than the window of 128 pixels on one axis"),
       (dict(canvas_window=64), (164, 64), "multiples of 8"),
       (dict(canvas_window=64), (160, 68), "multiples of 8"),
       (dict(canvas_window=64, canvas_stride=8), (160, 136), "more than 64"),         # 10 x 13 windows
       ]


@pytest.mark.parametrize("kw, size, match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_every_value_error_of_the_public_face(rig, kw, size, match):      # noqa: F811
    tools = _tools()
    with pytest.raises(ValueError, match=match):
        rig.pw.paint_with_words(dict(CONTEXT), _wide_map(size[1], size[0]), PROMPT, **rig.kw(tools, **kw))
    assert rig.events == [] and rig.encodes == []                          # before the conditioning and the sampler


def test_keywords_and_their_defaults():
    import paint_with_words as pw
    params = inspect.signature(pw.paint_with_words).parameters
    names = list(params)
    at = names.index("canvas_window")
    assert names[at:at + 3] == ["canvas_window", "canvas_stride", "canvas_ramp"] and at > names.index("strength")      # behind the reference's own
    assert params["canvas_window"].default is None and params["canvas_stride"].default is None and params["canvas_ramp"].default == 0
    doc = pw.paint_with_words.__doc__
    assert "canvas_window" in doc and "per window" in doc and "pipeline classes" in doc
    inp = __import__("paint_with_words.paint_with_words_inpaint", fromlist=["x"])
    for f in (pw.paint_with_words_batch, inp.paint_with_words_inpaint, inp.paint_with_words_inpaint_batch):            # out of scope
        assert "canvas_window" not in inspect.signature(f).parameters


def test_the_default_call_makes_the_calls_of_today(rig):      # noqa: F811
    """The rig's sampler has the `sample` signature of before the feature: a `canvas` keyword would be a TypeError. The plain call, the call
    with the keywords at their defaults, a window with a map no larger than it, and a stride / ramp without a window all hand the
    conditioning layer and the sampler the same things."""
    tools = _tools()
    calls = []
    for kw in ({}, dict(canvas_window=None, canvas_stride=None, canvas_ramp=0), dict(canvas_window=64), dict(canvas_window=128, canvas_stride=8, canvas_ramp=4),
               dict(canvas_stride=32, canvas_ramp=3)):
        ctx, neg = dict(CONTEXT), dict(NEG)
        lat = rig.pw.paint_with_words(ctx, _color_map(), PROMPT, seed=3, negative_color_context=neg, return_latents=True, **rig.kw(tools, **kw))
        e, s = rig.encodes[-1], rig.last()
        assert e["color_context"] is ctx and e["negative_color_context"] is neg and ctx == STRIPPED and neg == NEG_STRIPPED and lat is s.latents
        assert e["color_map_image"].size == (SIDE, SIDE) and tuple(s.latents.shape) == (1, 4, 8, 8) and isinstance(s.cond, dict)
        calls.append((dict(e, color_context=None, negative_color_context=None, text_encoder=None, tokenizer=None, color_map_image=None), s))
    assert len(rig.encodes) == len(calls) == 5 and rig.stripped == []
    first = calls[0]
    for e, s in calls[1:]:
        assert e == first[0]
        assert torch.equal(s.latents, first[1].latents) and torch.equal(s.timesteps, first[1].timesteps)
        assert (s.guidance_scale, s.extra_channels, s.on_step, s.negative_strength) == (7.5, None, None, 1.0)
        assert torch.equal(s.cond["CONTEXT_TENSOR"], first[1].cond["CONTEXT_TENSOR"]) and set(s.cond) == set(first[1].cond)


class _CanvasSampler:
    """Records what reaches `sample` (with the keywords of today) and hands the latents back."""
    calls = []

    def __init__(self, unet, scheduler, mode):
        self.mode = mode

    def sample(self, cond, uncond, latents, timesteps, guidance_scale, weight_function, extra_channels=None, on_step=None, negative_strength=1.0,
               regions=None, lora_rows=None, canvas=None):
        _CanvasSampler.calls.append(SimpleNamespace(cond=cond, uncond=uncond, latents=latents, timesteps=timesteps, regions=regions, lora_rows=lora_rows,
                                                    canvas=canvas, extra_channels=extra_channels, negative_strength=negative_strength))
        return latents

    def checked(self, latents):
        return latents


def test_cropped_color_maps_are_what_each_window_receives(rig, monkeypatch):      # noqa: F811
    from pww_hip import ops
    monkeypatch.setattr(rig.pw, "PwWSampler", _CanvasSampler)
    monkeypatch.setattr(ops, "region_masks", R.cpu_region_masks)
    _CanvasSampler.calls = []
    tools = _tools()
    rgb = C.color_map(96, 88)                                                  # case (b): ys = 0, 4; xs = 0, 3 -- an odd origin crops at pixel 24
    ys, xs = C.grid(12, 11, 8, 4)
    want = C.crops(rgb, ys, xs, 8, 8)
    ctx, neg = dict(CONTEXT), dict(NEG)
    regions = {(13, 255, 0): "a tree", (90, 206, 255): ("the sky", 0.5, 3.0)}
    lat = rig.pw.paint_with_words(ctx, Image.fromarray(rgb), PROMPT, seed=3, return_latents=True, canvas_window=64, canvas_ramp=3, region_prompts=regions,
                                  region_feather=1.0, **rig.kw(tools))
    # one parse at canvas size for the region seed of CONTEXT (no negative side), then one per window on its crop, tails still on
    assert len(rig.encodes) == 5 and rig.encodes[0]["color_map_image"].size == (88, 96) and rig.encodes[0]["negative_color_context"] is None
    for e, crop in zip(rig.encodes[1:], want):
        assert np.array_equal(np.asarray(e["color_map_image"]), crop) and e["color_context_before"] == CONTEXT and e["input_prompt"] == PROMPT
    assert all(e["color_context"] is not ctx for e in rig.encodes[:4]) and rig.encodes[4]["color_context"] is ctx and ctx == STRIPPED
    s = _CanvasSampler.calls[-1]
    assert s.canvas == {"size": (12, 11), "window": (8, 8), "ys": (0, 4), "xs": (0, 3), "ramp": 3}
    assert len(s.cond) == len(s.uncond) == len(s.regions) == 4 and tuple(s.latents.shape) == (1, 4, 12, 11) and lat is s.latents
    assert len({id(c) for c in s.cond}) == 4 and s.extra_channels is None and s.lora_rows is None
    for plan, crop in zip(s.regions, want):                                    # region masks and their feather: formed on the crop
        assert tuple(plan["masks"].shape) == (2, 8, 8) and len(plan["contexts"]) == 2
        assert np.array_equal(plan["masks"].numpy(), R.region_masks(crop, list(regions), 1.0))
        assert plan["scales"].tolist() == [7.5, 3.0]
    # the weight maps of a window are the maps of its crop: the window at (4, 3) against the plain call on that crop
    rig.pw.paint_with_words(dict(CONTEXT), Image.fromarray(want[3]), PROMPT, seed=3, return_latents=True, **rig.kw(tools))
    alone = _CanvasSampler.calls[-1].cond
    for key in [k for k in dict.keys(alone) if k.startswith("CROSS_ATTENTION_WEIGHT_") and k != "CROSS_ATTENTION_WEIGHT_ORIG"]:
        assert torch.equal(s.cond[3][key], alone[key]), key
    assert not torch.equal(s.cond[0]["CROSS_ATTENTION_WEIGHT_64"], s.cond[3]["CROSS_ATTENTION_WEIGHT_64"])
    # the initial latent is formed at canvas size, region seed against the canvas map: black (seed 42) differs from the plain seed-3 latent
    plain = torch.randn((1, 4, 12, 11), generator=torch.manual_seed(3)) * tools[4].init_noise_sigma
    black = torch.from_numpy((rgb == 0).all(-1).reshape(12, 8, 11, 8).all(axis=(1, 3)))          # latent pixels wholly inside the black bands
    white = torch.from_numpy((rgb == 255).all(-1).reshape(12, 8, 11, 8).all(axis=(1, 3)))
    assert black.any() and white.any()
    assert not torch.equal(s.latents[0, :, black], plain[0, :, black]) and torch.equal(s.latents[0, :, white], plain[0, :, white])
    # negative regions: the last window parses the caller's dict, which loses its tail once; without a region seed nothing is parsed at canvas size
    n = len(rig.encodes)
    ctx2 = {(0, 0, 0): "cat,1.0", (255, 255, 255): "dog,1.5,-1,2.5"}
    rig.pw.paint_with_words(ctx2, Image.fromarray(C.color_map(64, 160)), PROMPT, negative_color_context=neg, negative_strength=0.5, return_latents=True,
                            canvas_window=64, canvas_stride=32, **rig.kw(tools))
    new = rig.encodes[n:]
    assert len(new) == 4 and [e["negative_color_context"] is neg for e in new] == [False, False, False, True] and neg == NEG_STRIPPED
    assert all(e["negative_maps"] for e in new) and ctx2 == STRIPPED
    s = _CanvasSampler.calls[-1]
    assert s.canvas["xs"] == (0, 4, 8, 12) and s.canvas["ys"] == (0,) and s.canvas["ramp"] == 0 and s.negative_strength == 0.5 and s.regions is None
    # a colour of the context that is absent from a window gives zero maps there
    bands = np.zeros((64, 160, 3), dtype=np.uint8)
    bands[:, 96:] = 255                                                        # white only under the windows at 8 and 12
    rig.pw.paint_with_words({(255, 255, 255): "dog,1.5"}, Image.fromarray(bands), PROMPT, return_latents=True, canvas_window=64, **rig.kw(tools))
    conds = _CanvasSampler.calls[-1].cond
    sums = [float(c["CROSS_ATTENTION_WEIGHT_64"].abs().sum()) for c in conds]
    assert sums[0] == 0.0 and sums[1] == 0.0 and sums[2] > 0.0 and sums[3] > 0.0


def test_the_sampler_refuses_what_a_canvas_does_not_support():
    """PwWSampler.sample(canvas=...) checks the plan against the latent before anything runs (no device needed to get that far)."""
    import pww_hip
    from pww_hip.sampler import PwWSampler, canvas_plan
    from gpu_util import uninstall_all
    vae, unet, text, tok, sch = cases.build_tools("tiny")
    try:
        sampler = PwWSampler(unet, sch, "eager")
        plan = canvas_plan((8, 20), 8, 4)
        sch.set_timesteps(2)
        args = ({}, {}, torch.zeros(1, 4, 8, 20), sch.timesteps, 7.5, cases.weight_fn_runner)
        with pytest.raises(ValueError, match="float16 or bfloat16"):
            sampler.sample(*args, canvas=plan)                                              # the stand-in UNet here is fp32
        with pytest.raises(ValueError, match="plan is for a \\(8, 20\\) latent"):
            sampler.sample({}, {}, torch.zeros(1, 4, 8, 24), *args[3:], canvas=plan)
        with pytest.raises(ValueError, match="one float32 canvas"):
            sampler.sample({}, {}, torch.zeros(2, 4, 8, 20), *args[3:], canvas=plan)
        with pytest.raises(ValueError, match="inpainting"):
            sampler.sample(*args, extra_channels=torch.zeros(1, 5, 8, 20), canvas=plan)
        with pww_hip.record_attention_maps():
            with pytest.raises(ValueError, match="record_attention_maps"):
                sampler.sample(*args, canvas=plan)
    finally:
        uninstall_all()


# ---- the restatements against each other, and the record against fresh runs of the oracle loop

def test_restatement_properties():
    g = torch.Generator().manual_seed(0)
    (Hc, Wc), win, stride = C.KERNEL_CASES["b"]
    ys, xs = C.grid(Hc, Wc, win, stride)
    assert (ys, xs) == ([0, 4], [0, 3])
    eps = torch.randn(2 * 4, 4, win, win, generator=g).to(torch.float16)
    # identical windows' predictions average to themselves whatever the ramp; one window is classifier-free guidance
    same = torch.cat([eps[:1]] * 4 + [eps[1:2]] * 4)
    canvas = torch.randn(4, Hc, Wc, generator=g)
    rows = C.gather(canvas, ys, xs, win, win, 1.0, 2, torch.float16)
    assert tuple(rows.shape) == (8, 4, 8, 8) and torch.equal(rows[:4], rows[4:]) and torch.equal(rows[3], canvas[:, 4:, 3:].to(torch.float16))
    assert list(C.ramp_weights(8, 3)) == [1, 2, 3, 3, 3, 3, 2, 1] and list(C.ramp_weights(8, 64)) == [1, 2, 3, 4, 4, 3, 2, 1] and list(C.ramp_weights(3, 0)) == [1, 1, 1]
    assert np.array_equal(C.combine(eps.numpy(), ys, xs, (Hc, Wc), 7.5, 1), C.combine(eps.numpy(), ys, xs, (Hc, Wc), 7.5, 0))
    assert not np.array_equal(C.combine(eps.numpy(), ys, xs, (Hc, Wc), 7.5, 3), C.combine(eps.numpy(), ys, xs, (Hc, Wc), 7.5, 0))
    one = C.combine(same[[0, 4]].numpy(), [0], [0], (8, 8), 7.5, 3)
    u, e = same[4].float().numpy(), same[0].float().numpy()
    assert np.array_equal(one, (u + np.float32(7.5) * (e - u)) * np.float32(1.0) / np.float32(1.0))
    # the corner pixel (0, 0) belongs to window 0 alone; pixel (5, 4) to all four
    out = C.combine(eps.numpy(), ys, xs, (Hc, Wc), 7.5, 0)
    f = eps.float().numpy()
    v = [f[4 + i] + np.float32(7.5) * (f[i] - f[4 + i]) for i in range(4)]
    assert np.array_equal(out[:, 0, 0], v[0][:, 0, 0])
    want = (((v[0][:, 5, 4] + v[1][:, 5, 1]) + v[2][:, 1, 4]) + v[3][:, 1, 1]) / np.float32(4.0)
    assert np.array_equal(out[:, 5, 4], want)


@pytest.mark.parametrize("name", list(C.LOOPS) + ["plain"])
def test_the_record_is_the_oracle_loop(name):
    """A loop is 8 steps of batch-1 fp32 evaluations of the tiny UNet on 8 x 8 windows: seconds on the CPU, so every record is re-run."""
    rec = C.recorded()
    fresh = C.oracle_canvas_loop(C.PLAIN, plain=True) if name == "plain" else C.oracle_canvas_loop(name)
    assert tuple(fresh.shape) == tuple(rec[name].shape) and torch.isfinite(fresh).all()
    d = rel_l2(fresh, rec[name])
    print("%s: fresh oracle loop vs the record rel-L2 %.3e" % (name, d))
    assert d <= C.GOLDEN_TOL


def test_the_fixture_discriminates():
    """The canvas result lies far from the plain whole-canvas result of the same seed -- at least four times the loosest cap the GPU loops are
    held to -- and so does the loop with region prompts from the one without."""
    rec = C.recorded()
    visible = rel_l2(rec[C.PLAIN], rec["plain"])
    with_regions = rel_l2(rec["a_regions"], rec["a"])
    print("canvas vs plain whole-canvas loop on %s: rel-L2 %.3f; region prompts on vs off on (a): %.3f" % (C.PLAIN, visible, with_regions))
    assert abs(visible - C.ORACLE_VISIBLE) <= 2e-3 and visible >= 4 * max(C.CAP.values())
    assert with_regions >= 4 * max(C.CAP.values())
