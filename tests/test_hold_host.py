"""Region strength -- a denoising strength per colour for img2img -- without a GPU: the keywords and their checks, the release rule against
the reference's img2img offset, what reaches the sampler, the side library's table row / header / exports / refusals, the recorded oracle
loops, and the stand-alone host check under the sanitizers. The kernels and the loops on the device are tests/test_hold_gpu.py."""
import ctypes
import importlib
import inspect
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import hold_cases as H
import pww_cases as cases
from host_standins import cpu_masks  # noqa: F401  (fixture)
from test_entry_points_host import rig, _tools, _color_map, _init_image, _mask, CONTEXT, PROMPT, SIDE  # noqa: F401  (rig: fixture)

REPO, PKG = cases.REPO, cases.PKG
BLACK, WHITE, GREEN = (0, 0, 0), (255, 255, 255), (13, 255, 0)        # the colours of _color_map()


def _init(side=SIDE):
    return _init_image(side)


# ---- the keywords

def test_keywords_defaults_and_pipeline_attributes():
    import paint_with_words as pw
    from paint_with_words import pipelines
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    for f in (pw.paint_with_words, pw.paint_with_words_batch):
        params = inspect.signature(f).parameters
        names = list(params)
        at = names.index("negative_strength")
        assert names[at + 1:at + 5] == ["region_strength", "region_strength_feather", "lora", "region_loras"]
        assert params["region_strength"].default is None and params["region_strength_feather"].default == 0.0
        assert "region_strength" in f.__doc__ and "region_strength_feather" in f.__doc__
    doc = " ".join(pw.paint_with_words.__doc__.split())
    assert "Differential Diffusion" in doc and "bit for bit" in doc
    for f in (inp.paint_with_words_inpaint, inp.paint_with_words_inpaint_batch):
        assert not [n for n in inspect.signature(f).parameters if n.startswith("region_strength")]
    P = pipelines.PaintWithWord_StableDiffusionPipeline
    assert P.region_strength is None and P.region_strength_feather == 0.0
    for cls in (P, pipelines.PaintWithWord_StableDiffusionInpaintPipeline):
        assert not [n for n in inspect.signature(cls.__call__).parameters if n.startswith("region_strength")]      # the call signature is pinned


# ---- every ValueError of the public face, before the tools are touched

NAN = float("nan")
NINE = {(i, i, i): 0.5 for i in range(9)}
BAD = [
    (dict(region_strength={BLACK: 0.2}), "need an init image"),
    (dict(region_strength_feather=1.0), "need an init image"),
    (dict(region_strength={BLACK: 1.5}, init=True), r"must be in \[0, 1\]"),
    (dict(region_strength={BLACK: -0.1}, init=True), r"must be in \[0, 1\]"),
    (dict(region_strength={BLACK: NAN}, init=True), "finite number"),
    (dict(region_strength={BLACK: "0.5"}, init=True), "finite number"),
    (dict(region_strength={BLACK: True}, init=True), "finite number"),
    (dict(region_strength=NINE, init=True), "1 to 8 colours"),
    (dict(region_strength={BLACK: 0.5, "#000000": 0.7}, init=True), "twice"),
    (dict(region_strength={(0, 0): 0.5}, init=True), "region_strength: colour"),
    (dict(region_strength={"black": 0.5}, init=True), "region_strength: colour"),
    (dict(region_strength=[{BLACK: 0.5}], init=True), "must be a dict"),
    (dict(region_strength=0.5, init=True), "must be a dict"),
    (dict(region_strength={BLACK: 0.5}, region_strength_feather=8.5, init=True), r"region_strength_feather must be in \[0, 8\]"),
    (dict(region_strength={BLACK: 0.5}, region_strength_feather=-1.0, init=True), "region_strength_feather"),
    (dict(region_strength={BLACK: 0.5}, region_strength_feather=NAN, init=True), "region_strength_feather"),
    (dict(region_strength={BLACK: 0.5}, strength=1.5, init=True), "`strength`"),
    (dict(region_strength={BLACK: 0.5}, strength=NAN, init=True), "`strength`"),
    (dict(region_strength={BLACK: 0.0}, strength=0.0, init=True), "nothing would be denoised"),          # i0 = T
    (dict(region_strength={BLACK: 0.3}, strength=0.2, init=True), "nothing would be denoised"),          # 3 steps: theta_2 = 1 / 3 > 0.3
    (dict(region_strength={BLACK: 0.5}, init=128), "8 x the latent"),                                  # a 128-pixel init image under a 64-pixel map
    (dict(region_strength={BLACK: 0.5}, init=(96, 64)), "8 x the latent"),
]


@pytest.mark.parametrize("kw, match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_every_value_error_of_the_public_face(rig, kw, match):      # noqa: F811
    kw = dict(kw)
    init = kw.pop("init", None)
    if init is not None:
        kw["init_image"] = _init() if init is True else _init(init) if isinstance(init, int) else Image.new("RGB", init)
    tools = _tools()
    with pytest.raises(ValueError, match=match):
        rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, **rig.kw(tools, **kw))
    batch = {("init_images" if k == "init_image" else k): v for k, v in kw.items()}
    if isinstance(batch.get("region_strength"), list):
        batch["region_strength"] = batch["region_strength"] * 3          # the batch form takes a sequence: one per seed, not three for two
        match = "3 entries for 2 requests"
    with pytest.raises(ValueError, match=match):
        rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1], **rig.kw(tools, **batch))
    assert rig.events == [] and rig.encodes == []                          # before the conditioning and the sampler


def test_schedulers_that_are_refused(rig):      # noqa: F811
    from sd_standin import PLMSScheduler, LMSDiscreteScheduler

    class NoAddNoise(LMSDiscreteScheduler):
        @property
        def add_noise(self):
            raise AttributeError("add_noise")
    for sch, match in ((PLMSScheduler(), "steps_offset = 1"),
                       (NoAddNoise(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000), "add_noise")):
        tools = _tools()[:4] + (sch,)
        with pytest.raises(ValueError, match=match):
            rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, init_image=_init(), region_strength={BLACK: 0.2}, **rig.kw(tools))
        assert rig.events == [] and rig.encodes == []


def test_the_inpaint_faces_reject_the_keyword(rig):      # noqa: F811
    tools = _tools(9)
    with pytest.raises(TypeError, match="region_strength"):
        rig.inp.paint_with_words_inpaint(dict(CONTEXT), _color_map(), _mask(), _init(128), PROMPT, region_strength={BLACK: 0.5}, **rig.kw(tools))
    with pytest.raises(TypeError, match="region_strength"):
        rig.inp.paint_with_words_inpaint_batch(dict(CONTEXT), _color_map(), _mask(), _init(128), PROMPT, [0], region_strength={BLACK: 0.5}, **rig.kw(tools))
    vae, unet, text, tok, _ = tools
    pipe = rig.pipes.PaintWithWord_StableDiffusionInpaintPipeline(vae, text, tok, unet)
    for attr, value in (("region_strength", {BLACK: 0.5}), ("region_strength_feather", 1.0)):
        setattr(pipe, attr, value)
        with pytest.raises(ValueError, match="not part of the inpaint pipeline"):
            pipe(PROMPT, image=_init(), mask_image=_mask(), color_map_image=_color_map(), color_context=dict(CONTEXT), num_inference_steps=3)
        delattr(pipe, attr)
    assert rig.count("sample") == 0 and rig.encodes == []
    plain = rig.pipes.PaintWithWord_StableDiffusionPipeline(vae, text, tok, _tools()[1])
    plain.region_strength = {BLACK: 0.5}
    with pytest.raises(ValueError, match="need an init image"):
        plain(PROMPT, color_map_image=_color_map(), color_context=dict(CONTEXT), num_inference_steps=3)
    assert rig.count("sample") == 0 and rig.encodes == []


# ---- the release rule

def test_thresholds_and_first_against_the_reference_rule():
    from pww_hip import sampler as S
    pairs = H.grid_pairs()
    assert len(pairs) > 1500 and {T for T, _ in pairs} == set(H.STEP_COUNTS)
    disagree = []
    for T in H.STEP_COUNTS:
        theta = S.hold_thresholds(T)
        assert len(theta) == T + 1 and theta[0] == 1.0 and theta[T] == 0.0
        assert all(isinstance(v, float) and np.float32(v) == v for v in theta)                    # exact fp32 values
        assert [np.float32(v) for v in theta] == H.thresholds(T)
        assert all(a > b for a, b in zip(theta, theta[1:]))
    for T, s in pairs:
        g = S.hold_first(T, s)
        assert g == H.first(T, s)
        assert g == T or np.float32(s) >= np.float32(S.hold_thresholds(T)[g])
        assert g == 0 or np.float32(s) < np.float32(S.hold_thresholds(T)[g - 1])                 # the smallest such step
        if g != H.reference_first(T, s):
            disagree.append((T, s))
    assert tuple(disagree) == H.DISAGREE
    # the pairs the tests compare with the plain call on agree
    for T, s in [(8, 0.25), (8, 0.5), (8, 0.75), (8, 1.0), (30, 0.5), (30, 0.7)]:
        assert S.hold_first(T, s) == H.reference_first(T, s)
    assert S.hold_first(8, 0.125) == 7 and S.hold_first(8, 0.12) == 8 and S.hold_first(8, 0.0) == 8       # equality releases; below theta_7 nothing does
    with pytest.raises(ValueError):
        S.hold_first(8, 1.5)
    with pytest.raises(ValueError):
        S.hold_thresholds(0)


def test_the_four_known_disagreements_are_pinned():
    """In these four the reference's double product T * s lands one ulp under an integer, so its int() drops a step that the rule keeps."""
    from pww_hip import sampler as S
    for T, s in H.DISAGREE:
        assert T * s < round(T * s) and round(T * s) - T * s < 1e-13
        assert S.hold_first(T, s) == T - round(T * s) == H.reference_first(T, s) - 1


def test_the_table_of_a_request():
    """(theta, a, b) per step: theta_{g + 1} with the LMS stand-in's (1, sigma_{g + 1}); behind the last step theta_{T - 1} and (1, 0)."""
    from pww_hip import sampler as S
    sch = _tools()[4]
    T, i0 = 8, 2
    sch.set_timesteps(T)
    me = SimpleNamespace(scheduler=sch)
    me._hold_coefficients = lambda t: S.PwWSampler._hold_coefficients(me, t)
    lat = torch.zeros(2, 4, 8, 8)
    hold = {"init": lat.clone(), "noise": lat.clone(), "strength": torch.zeros(2, 8, 8), "steps": T, "first": i0}
    table = S.PwWSampler._hold_table(me, hold, lat, sch.timesteps[i0:], None)
    theta = H.thresholds(T)
    assert len(table) == T - i0
    for i, (th, a, b) in enumerate(table[:-1]):
        assert np.float32(th) == theta[i0 + i + 1] and a == 1.0 and b == float(sch.sigmas[i0 + i + 1])
    assert table[-1] == (float(theta[T - 1]), 1.0, 0.0)
    for bad, match in ((dict(first=8), "timesteps do not go"), (dict(steps=9), "timesteps do not go"), (dict(strength=torch.zeros(2, 4, 8, 8)), "strength map"),
                       (dict(noise=lat.double()), "float32"), (dict(init=lat[:1]), "init latent")):
        with pytest.raises(ValueError, match=match):
            S.PwWSampler._hold_table(me, dict(hold, **bad), lat, sch.timesteps[i0:], None)
    with pytest.raises(ValueError, match="inpainting"):
        S.PwWSampler._hold_table(me, hold, lat, sch.timesteps[i0:], torch.zeros(2, 5, 8, 8))
    sch.add_noise = lambda x, n, t: x + n + x * n                # not a x0 + b z: 1, 1 and 3
    with pytest.raises(ValueError, match="not a x0"):
        S.PwWSampler._hold_table(me, hold, lat, sch.timesteps[i0:], None)


# ---- what reaches the sampler

def test_the_default_call_makes_the_calls_of_today(rig):      # noqa: F811
    """The rig's sampler has the `sample` signature of before the feature: a `hold` keyword would be a TypeError. img2img with the keywords
    absent, at their defaults and with an empty dict hands the sampler the same things."""
    tools = _tools()
    calls = []
    for kw in ({}, dict(region_strength=None, region_strength_feather=0.0), dict(region_strength={}), dict(region_strength_feather=0)):
        torch.manual_seed(11)
        lat = rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, init_image=_init(), strength=0.7, return_latents=True, **rig.kw(tools, **kw))
        s = rig.last()
        assert lat is s.latents and tuple(lat.shape) == (1, 4, 8, 8)
        calls.append(s)
    torch.manual_seed(11)
    rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0], init_images=_init(), strength=0.7, return_latents=True,
                                  **rig.kw(tools, region_strength=[None], region_strength_feather=0.0))
    calls.append(rig.last())
    for s in calls[1:]:
        assert torch.equal(s.latents, calls[0].latents) and torch.equal(s.timesteps, calls[0].timesteps) and len(s.timesteps) == 2      # 3 steps at 0.7
        assert (s.guidance_scale, s.extra_channels, s.on_step, s.negative_strength) == (7.5, None, None, 1.0)
        assert torch.equal(s.cond["CONTEXT_TENSOR"], calls[0].cond["CONTEXT_TENSOR"]) and set(s.cond) == set(calls[0].cond)


class _HoldSampler:
    """Records what reaches `sample` (today's keywords and `hold`) and hands the latents back."""
    calls = []

    def __init__(self, unet, scheduler, mode):
        pass

    def sample(self, cond, uncond, latents, timesteps, guidance_scale, weight_function, extra_channels=None, on_step=None, negative_strength=1.0, hold=None):
        type(self).calls.append(SimpleNamespace(cond=cond, latents=latents, timesteps=timesteps, hold=hold))
        return latents

    def checked(self, latents):
        return latents

    def check_errors(self):
        pass


@pytest.fixture
def hold_rig(rig, monkeypatch):      # noqa: F811
    """The rig with a sampler that takes `hold`, and the strength-map launch restated on the CPU (tests/hold_cases.py)."""
    from pww_hip import ops
    _HoldSampler.calls = []
    monkeypatch.setattr(rig.pw, "PwWSampler", _HoldSampler)
    monkeypatch.setattr(ops, "hold_strength_map", lambda rgb, colors, strengths, s0, feather=0.0: torch.from_numpy(
        H.strength_map(rgb.numpy(), colors, strengths, s0, feather)))
    return rig


def test_what_a_region_strength_request_hands_the_sampler(hold_rig):
    rig = hold_rig      # noqa: F811
    tools = _tools()
    T = 8
    torch.manual_seed(4)
    plain = rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, init_image=_init(), strength=0.75, return_latents=True,
                                    **rig.kw(tools, num_inference_steps=T))
    p = _HoldSampler.calls[-1]
    assert p.hold is None
    torch.manual_seed(4)
    strengths = {BLACK: 0.0, "#ffffff": 0.75, (1, 2, 3): 0.5}          # (1, 2, 3) is not in the map: it still counts for the first step
    lat = rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, init_image=_init(), strength=0.25, region_strength=strengths, return_latents=True,
                                  **rig.kw(tools, num_inference_steps=T))
    s = _HoldSampler.calls[-1]
    h = s.hold
    assert set(h) == {"init", "noise", "strength", "steps", "first"} and (h["steps"], h["first"]) == (T, 2)
    assert torch.equal(s.timesteps, p.timesteps) and len(s.timesteps) == 6          # first(0.75) of 8 steps = 2: the plain call's tail at 0.75
    assert torch.equal(lat, plain)                                                  # the same start: a_2 x0 + b_2 z with the same z
    sch = tools[4]
    assert torch.equal(lat, sch.add_noise(h["init"], h["noise"], s.timesteps[:1]))
    want = H.strength_map(np.array(_color_map()), [BLACK, WHITE, (1, 2, 3)], [0.0, 0.75, 0.5], 0.25)
    assert tuple(h["strength"].shape) == (1, 8, 8) and np.array_equal(h["strength"][0].numpy(), want)
    assert want[0, 0] == 0.0 and want[0, 7] == 0.75 and want[3, 3] == np.float32(0.25) * 1 and 0.25 in want       # the green square keeps the base strength
    assert h["init"].dtype == h["noise"].dtype == h["strength"].dtype == torch.float32 and h["init"].shape == h["noise"].shape == lat.shape
    # the pipeline class: eta is the base strength, the attributes carry the rest
    vae, unet, text, tok, _ = tools
    pipe = rig.pipes.PaintWithWord_StableDiffusionPipeline(vae, text, tok, _tools()[1])
    pipe.region_strength, pipe.region_strength_feather = {WHITE: 1.0}, 2.0
    pipe(PROMPT, color_map_image=_color_map(), color_context=dict(CONTEXT), image=_init(), eta=0.5, num_inference_steps=T, output_type="np")
    h = _HoldSampler.calls[-1].hold
    assert (h["steps"], h["first"]) == (T, 0) and len(_HoldSampler.calls[-1].timesteps) == T
    assert np.array_equal(h["strength"][0].numpy(), H.strength_map(np.array(_color_map()), [WHITE], [1.0], 0.5, 2.0))


def test_batch_forms(hold_rig):
    rig = hold_rig      # noqa: F811
    tools = _tools()
    T = 8
    kw = dict(init_images=_init(), strength=0.25, return_latents=True)
    # one dict for all requests
    rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1, 2], region_strength={BLACK: 0.5}, **kw, **rig.kw(tools, num_inference_steps=T))
    s = _HoldSampler.calls[-1]
    assert (s.hold["steps"], s.hold["first"]) == (T, 4) and len(s.timesteps) == 4 and tuple(s.hold["strength"].shape) == (3, 8, 8)
    assert torch.equal(s.hold["strength"][0], s.hold["strength"][2]) and tuple(s.hold["init"].shape) == tuple(s.hold["noise"].shape) == (3, 4, 8, 8)
    assert not torch.equal(s.hold["noise"][0], s.hold["noise"][1])                   # drawn per image from the global generator
    # one per seed, with a None and an empty dict: the first step comes from the largest strength of ALL requests
    per = [{BLACK: 0.5}, None, {WHITE: 0.75, BLACK: 0.0}, {}]
    rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1, 2, 3], region_strength=per, **kw, **rig.kw(tools, num_inference_steps=T))
    s = _HoldSampler.calls[-1]
    assert (s.hold["steps"], s.hold["first"]) == (T, 2) and len(s.timesteps) == 6
    S = s.hold["strength"].numpy()
    rgb = np.array(_color_map())
    assert np.array_equal(S[0], H.strength_map(rgb, [BLACK], [0.5], 0.25)) and np.array_equal(S[2], H.strength_map(rgb, [WHITE, BLACK], [0.75, 0.0], 0.25))
    assert (S[1] == np.float32(0.25)).all() and (S[3] == np.float32(0.25)).all()
    # all None: the call of before
    rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1], region_strength=[None, {}], **kw, **rig.kw(tools, num_inference_steps=T))
    assert _HoldSampler.calls[-1].hold is None and len(_HoldSampler.calls[-1].timesteps) == 2
    with pytest.raises(ValueError, match="2 entries for 3 requests"):
        rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1, 2], region_strength=[None, {}], **kw, **rig.kw(tools))


# ---- the side library: table row, header, exports

def test_the_table_row_header_and_exports(built_lib):
    import build as pww_build
    from pww_hip import _lib
    assert "hold" in _lib.SIDE_EXTRA and tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA)
    spec = _lib.side_spec("hold")
    assert spec is _lib.SIDE_EXTRA["hold"] and set(spec) == set(_lib.SIDE["regions"]) and not spec["missing_ok"]
    assert spec["exports"] is _lib.HOLD_EXPORTS and spec["min_version"] == _lib.HOLD_MIN_VERSION == 100 and spec["path"] == "HOLD_LIB_PATH"
    assert _lib.HOLD_LIB_PATH.endswith("libpww_hip_hold.so") and "PWW_HIP_HOLD_LIB" in inspect.getsource(_lib)
    assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_hold_version", "pww_hold_last_error"}
    assert {"pww_hold_strength_map", "pww_hold_feather", "pww_hold_apply"} <= set(spec["exports"])
    assert pww_build.SIDE_LIBS_EXTRA["hold"][0] == "pww_hold.hip" and "-fvisibility=hidden" in pww_build.SIDE_UNITS["hold"][0][1]
    assert pww_build.PER_FILE_FLAGS["pww_hold.hip"] == ["-ffp-contract=off"] and pww_build.LIB_HOLD == pww_build.SIDE_PATHS["hold"]
    assert "hold " in pww_build.__doc__
    header = open(REPO + "/include/pww_hip_hold.h").read()
    assert "#define PWW_HOLD_VERSION 100" in header and "#define PWW_HOLD_MAX_COLORS 8" in header and "#define PWW_HOLD_MAX_FEATHER 8.0f" in header
    assert (_lib.HOLD_MAX_COLORS, _lib.HOLD_MAX_FEATHER, _lib.HOLD_MAX_RADIUS) == (8, 8.0, 24) and "#define PWW_HOLD_MAX_RADIUS 24" in header
    for fn in spec["exports"]:
        assert "%s(" % fn in header
    source = open(PKG + "/csrc/pww_hold.hip").read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_hold"' in source
    assert "atomic" not in source and "__fmaf" not in source and "fmaf(" not in source


@pytest.fixture(scope="module")
def hold_lib(built_lib):
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_hold()
    return _lib.load_side("hold")


def test_a_real_load_binds_the_entry_points(hold_lib):
    from pww_hip import _lib
    assert hold_lib is not None and _lib.load_hold() is hold_lib and hold_lib.pww_hold_version() == 100
    for fn, (argtypes, restype) in _lib.SIDE_EXTRA["hold"]["sigs"].items():
        assert getattr(hold_lib, fn).argtypes == argtypes and getattr(hold_lib, fn).restype is restype, fn
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.HOLD_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in dyn.splitlines() if " T " in line and not line.split()[-1].startswith(("_init", "_fini")))
    assert visible == sorted(_lib.HOLD_EXPORTS)          # -fvisibility=hidden: the entry points and nothing else


def test_a_missing_file_is_an_error(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "hold", None)
    monkeypatch.setattr(_lib, "HOLD_LIB_PATH", str(tmp_path / "libpww_hip_hold.so"))
    with pytest.raises(_lib.PwwHipError, match="libpww_hip_hold.so not found .*rebuild"):
        _lib.load_hold()


def test_the_host_tables_of_the_library(hold_lib):
    """pww_hold_thresholds is sampler.hold_thresholds; pww_hold_taps are the taps the restatement of the feather uses."""
    from pww_hip import sampler as S
    for T in H.STEP_COUNTS:
        buf = (ctypes.c_float * (T + 1))()
        assert hold_lib.pww_hold_thresholds(T, buf) == 0 and list(buf) == S.hold_thresholds(T)
    for sigma in (0.5, 2.0, 8.0):
        buf = (ctypes.c_float * 25)()
        radius = hold_lib.pww_hold_taps(sigma, buf, 25)
        assert radius == int(np.ceil(3.0 * sigma))
        want = np.exp(-0.5 * (np.arange(radius + 1, dtype=np.float64) / sigma) ** 2).astype(np.float32)
        assert np.array_equal(np.array(buf[:radius + 1], dtype=np.float32), want)


# ---- every refusal of the entry points, in front of the first HIP runtime call

P, Q, NULL = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0)        # never dereferenced: validation precedes every launch
EINVAL, ENOTSUP = -22, -95
INF = float("inf")


def _map(lib, rgb=P, colors=(0, 0, 0), deltas=(0.25,), s0=0.5, out=P, H_=64, W=64, K=1):
    c = None if colors is None else (ctypes.c_uint8 * len(colors))(*colors)
    d = None if deltas is None else (ctypes.c_float * len(deltas))(*deltas)
    return lib.pww_hold_strength_map(rgb, c, d, s0, out, H_, W, K, None)


def _feather(lib, src=P, tmp=Q, out=P, h=8, w=8, sigma=1.0):
    return lib.pww_hold_feather(src, tmp, out, h, w, sigma, None)


def _apply(lib, x=P, x0=P, z=P, S=P, theta=0.5, a=1.0, b=1.0, n=1, C=4, hw=64):
    return lib.pww_hold_apply(x, x0, z, S, theta, a, b, n, C, hw, None)


REFUSALS = {
    "strength_map": (_map, [
        (dict(rgb=NULL), EINVAL, "null"), (dict(colors=None), EINVAL, "null"), (dict(deltas=None), EINVAL, "null"), (dict(out=NULL), EINVAL, "null"),
        (dict(K=0), EINVAL, "0 colours"), (dict(K=9, colors=(0,) * 27, deltas=(0.0,) * 9), EINVAL, "9 colours"), (dict(H_=7), EINVAL, "smaller than one latent pixel"),
        (dict(W=4), EINVAL, "smaller than one latent pixel"), (dict(s0=NAN), EINVAL, "base strength"), (dict(s0=INF), EINVAL, "base strength"),
        (dict(deltas=(NAN,)), EINVAL, "colour 0"), (dict(K=2, colors=(0,) * 6, deltas=(0.0, -INF)), EINVAL, "colour 1"),
        (dict(H_=1 << 20, W=1 << 20), ENOTSUP, "2^31")]),
    "feather": (_feather, [
        (dict(src=NULL), EINVAL, "null"), (dict(tmp=NULL), EINVAL, "null"), (dict(out=NULL), EINVAL, "null"), (dict(tmp=P), EINVAL, "of its own"),
        (dict(out=Q), EINVAL, "of its own"), (dict(h=0), EINVAL, "bad size"), (dict(w=-3), EINVAL, "bad size"), (dict(sigma=-1.0), EINVAL, "sigma"),
        (dict(sigma=8.5), EINVAL, "sigma"), (dict(sigma=NAN), EINVAL, "sigma"), (dict(sigma=INF), EINVAL, "sigma"), (dict(h=1 << 16, w=1 << 16), ENOTSUP, "2^31")]),
    "apply": (_apply, [
        (dict(x=NULL), EINVAL, "null"), (dict(x0=NULL), EINVAL, "null"), (dict(z=NULL), EINVAL, "null"), (dict(S=NULL), EINVAL, "null"),
        (dict(n=0), EINVAL, "bad size"), (dict(C=0), EINVAL, "bad size"), (dict(hw=0), EINVAL, "bad size"), (dict(hw=-4), EINVAL, "bad size"),
        (dict(theta=NAN), EINVAL, "finite"), (dict(theta=INF), EINVAL, "finite"), (dict(a=NAN), EINVAL, "finite"), (dict(a=-INF), EINVAL, "finite"),
        (dict(b=NAN), EINVAL, "finite"), (dict(b=INF), EINVAL, "finite"), (dict(C=1024, hw=1 << 30), ENOTSUP, "2^40"), (dict(n=4, C=1, hw=1 << 29), ENOTSUP, "2^31")]),
}


@pytest.mark.parametrize("entry", list(REFUSALS))
def test_every_refusal_returns_before_a_hip_call_and_fills_the_error_slot(hold_lib, entry):
    from pww_hip import _lib
    call, cases_ = REFUSALS[entry]
    product = _lib.load()
    before = product.pww_last_error()
    for kw, want, word in cases_:
        rc = call(hold_lib, **kw)
        text = hold_lib.pww_hold_last_error().decode()
        assert rc == want, (kw, rc, text)
        assert text.startswith("hold_%s: " % entry) and word in text, (kw, text)
        with pytest.raises(_lib.PwwHipError) as e:
            _lib.check(rc, "pww_hold_" + entry, hold_lib)
        assert text in str(e.value) and "rc=%d" % want in str(e.value)
    assert product.pww_last_error() == before               # the product library's slot is another one


def test_ops_argument_checks():
    """In the style of region_masks and canvas_combine: a CPU tensor, a wrong type or shapes that do not go together raise before the
    library is asked."""
    from pww_hip import ops
    from pww_hip._lib import PwwHipError
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.hold_apply(x, x, x, torch.zeros(1, 8, 8), 0.5, 1.0, 1.0)
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.hold_strength_map(torch.zeros(64, 64, 3, dtype=torch.uint8), [BLACK], [0.5], 0.5)
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.hold_feather(torch.zeros(8, 8), 1.0)


def test_the_validation_paths_under_the_sanitizers(tmp_path):
    """tests/native/hold_host_check.cpp + csrc/pww_hold.hip as ONE stand-alone program, host code under -fsanitize=address,undefined (nothing
    is loaded into this interpreter): every refusal again, the tap and threshold tables, and the sanitizers must stay silent."""
    import build as pww_build
    exe = str(tmp_path / "hold_host_check")
    cmd = [pww_build.HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "native", "hold_host_check.cpp"),
           os.path.join(PKG, "csrc", "pww_hold.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    # (the HIP runtime's process-lifetime allocations are not this library's: the leak pass is off, every other check is on)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and "hold_host_check OK" in run.stdout, run.stdout + run.stderr
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr


# ---- the restatements and the recorded loops

def test_restatement_properties():
    rgb = H.map_rgb(64, 64, H.COLORS8)
    S = H.strength_map(rgb, H.COLORS8, H.STRENGTHS8, 0.5)
    assert S.dtype == np.float32 and S.shape == (8, 8) and S.min() >= 0 and S.max() <= 1
    assert np.array_equal(H.strength_map(rgb, H.COLORS8, [0.5] * 8, 0.5), np.full((8, 8), 0.5, dtype=np.float32))          # every delta 0
    assert np.array_equal(H.strength_map(rgb, [(9, 9, 9)], [1.0], 0.25), np.full((8, 8), 0.25, dtype=np.float32))           # a colour that is absent
    one = H.map_rgb(64, 64, H.COLORS8, single=H.COLORS8[2])
    assert np.array_equal(H.strength_map(one, H.COLORS8, H.STRENGTHS8, 0.5), np.full((8, 8), H.STRENGTHS8[2], dtype=np.float32))
    F = H.feather(S, 2.0)
    assert F.min() >= 0 and F.max() <= 1 and not np.array_equal(F, S) and np.array_equal(H.feather(np.full((9, 5), 0.25, np.float32), 8.0), np.full((9, 5), 0.25, np.float32))
    x, x0, z, Sm = H.apply_inputs(1, 4, 64)
    out = H.apply(x, x0, z, Sm, 0.5, 1.0, 0.0)
    held = Sm < 0.5
    assert np.array_equal(out[0][:, held[0]], x0[0][:, held[0]]) and np.array_equal(out[0][:, ~held[0]], x[0][:, ~held[0]], equal_nan=True)
    assert not held[0, 4] and held[0, 3]                                            # S = 4 / 8 = theta releases
    assert np.array_equal(H.apply(x, x0, z, Sm, 0.0, 1.0, 1.0), x, equal_nan=True) and np.isfinite(H.apply(x, x0, z, Sm, 1.5, 0.6, 0.8)).all()


@pytest.fixture(scope="module")
def oracle_latents():
    return H.recorded()


@pytest.mark.parametrize("name", list(H.LOOPS))
def test_the_record_is_the_oracle_loop(oracle_latents, name):
    trace = []
    fresh = H.oracle_hold_loop(name, trace=trace)
    assert tuple(fresh.shape) == tuple(oracle_latents[name].shape) and H.rel(fresh, oracle_latents[name]) <= H.GOLDEN_TOL
    if name == "half_keep":
        x0 = H.init_latent(name)
        assert len(trace) == 6                                                       # first(0.75) of 8 steps = 2: six steps, six holds
        assert torch.equal(fresh[..., :4], x0[..., :4]) and torch.equal(oracle_latents[name][..., :4], x0[..., :4])        # the s = 0 half is x0, bit for bit
        assert H.rel(fresh[..., 4:], x0[..., 4:]) > 0.1
    if name == "three":
        assert len(trace) == 8


def test_the_fixture_discriminates(oracle_latents):
    """The plain img2img loop at the largest strength lies far outside every cap from the loop that keeps half of the image."""
    d = H.rel(oracle_latents["plain"], oracle_latents["half_keep"])
    print("plain vs half_keep: rel-L2 %.3f" % d)
    assert d > 4 * max(H.CAP.values())
    assert H.rel(oracle_latents["three"], oracle_latents["half_keep"]) > 4 * max(H.CAP.values())
