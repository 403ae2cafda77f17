"""Step plans without a GPU: the seven-number table of pww_hip.steps against the published updates written out directly and against the
scheduler classes' own step(), all in float64 on the exact denoiser of Gaussian data; the order of convergence of the tables; `covers`;
the `sampler` keyword of the four function faces; the side library's table row, header, exports and refusals. The kernel and the loops on
the device are tests/test_steps_gpu.py."""
import ctypes
import importlib
import inspect
import math
import subprocess

import numpy as np
import pytest
import torch

import pww_cases as cases
import sched_cases as SC
from host_standins import cpu_masks  # noqa: F401  (fixture)
from test_entry_points_host import rig, _tools, _color_map, _init_image, _mask, CONTEXT, PROMPT  # noqa: F401  (rig: fixture)

REPO, PKG = cases.REPO, cases.PKG
TOL = 1e-12                   # an algebraic identity in float64 (3.2e-14 was the worst case when the form was derived)


# ---- 1. the table against the direct restatements and the classes

@pytest.mark.parametrize("T", [1, 2, 3, 10])
@pytest.mark.parametrize("karras", [False, True], ids=["linspace", "karras"])
@pytest.mark.parametrize("prediction", SC.PREDICTIONS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_table_against_direct_restatement_and_class(kind, prediction, karras, T):
    from pww_hip import steps
    sch = SC.make(kind, prediction, karras, T)
    ts = sch.timesteps
    n = len(ts)                                       # (DDIM on integer Karras timesteps may visit fewer than T)
    sig = SC.sigmas_of(sch, ts)
    rows = steps.rows64(sch, ts)
    assert rows.shape == (n, 7) and rows[0, 4] == 0.0 and np.isfinite(rows).all()
    zs = SC.noises(n)
    x0 = SC.start(kind, sig[0])
    table = SC.run_rows(kind, rows, sig, x0.clone(), prediction, zs)
    direct = SC.run_direct(kind, sch, ts, x0.clone(), prediction, zs)
    own = SC.run_class(SC.make(kind, prediction, karras, T), ts, x0.clone(), prediction)
    d_direct, d_own = SC.rel(table, direct), SC.rel(table, own)
    print("%s %s %s T=%d: table vs direct %.2e, vs step() %.2e" % (kind, prediction, "karras" if karras else "linspace", T, d_direct, d_own))
    assert d_direct <= TOL and d_own <= TOL
    # the plan is the table rounded once to fp32, as Python floats
    plan = steps.plan(sch, ts)
    assert len(plan) == n and all(len(r) == 7 and all(isinstance(v, float) for v in r) for r in plan)
    assert np.array_equal(np.asarray(plan, dtype=np.float64), rows.astype(np.float32).astype(np.float64))
    # what the rows say about the scheduler
    assert (rows[:, 5] != 0).any() == steps.stochastic(sch) or n == 1
    if kind in SC.SIGMA_SPACE:
        assert np.allclose(rows[:-1, 6], np.sqrt(np.asarray(sig[1:-1]) ** 2 + 1.0), rtol=0, atol=0) and rows[-1, 6] == 1.0
    else:
        assert (rows[:, 6] == 1.0).all()
    if kind == "dpmpp_2m":
        assert (rows[1:-1, 4] != 0).all() and tuple(rows[-1, 2:5]) == (0.0, 1.0, 0.0)      # history from the second step on; the last step returns q
    else:
        assert (rows[:, 4] == 0).all()


@pytest.mark.parametrize("prediction", SC.PREDICTIONS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_img2img_suffix_starts_without_history(kind, prediction):
    """6 of 10 steps: the first executed row has c = 0 whatever its index in the full schedule, and the three routes still agree."""
    from pww_hip import steps
    sch = SC.make(kind, prediction, False, 10)
    ts = sch.timesteps[4:]
    sig = SC.sigmas_of(sch, ts)
    rows = steps.rows64(sch, ts)
    full = steps.rows64(sch, sch.timesteps)
    assert rows.shape == (6, 7) and rows[0, 4] == 0.0
    assert np.array_equal(rows[1:], full[5:]) and np.array_equal(np.delete(rows[0], [3, 4]), np.delete(full[4], [3, 4]))
    if kind == "dpmpp_2m":
        assert full[4, 4] != 0.0 and rows[0, 3] != full[4, 3]
    zs = SC.noises(6)
    x0 = SC.start(kind, sig[0])
    table = SC.run_rows(kind, rows, sig, x0.clone(), prediction, zs)
    assert SC.rel(table, SC.run_direct(kind, sch, ts, x0.clone(), prediction, zs)) <= TOL
    assert SC.rel(table, SC.run_class(SC.make(kind, prediction, False, 10), ts, x0.clone(), prediction)) <= TOL


# ---- 2. order of convergence on Karras sigmas, the last jump to 0 left off

def _flow_error(kind, T):
    from pww_hip import steps
    sch = SC.make(kind, "epsilon", True, T)
    ts = sch.timesteps[:-1]
    sig = SC.sigmas_of(sch, ts)
    x0 = SC.start(kind, sig[0])
    got = SC.run_rows(kind, steps.rows64(sch, ts), sig, x0.clone(), "epsilon")
    return SC.rel(got, SC.exact_flow(kind, x0, sig[0], sig[-1]))


@pytest.mark.parametrize("kind, lo, hi", [("euler", 0.8, 1.2), ("ddim", 0.8, 1.2), ("dpmpp_2m", 1.8, None)])
def test_order_of_convergence(kind, lo, hi):
    e40, e80 = _flow_error(kind, 40), _flow_error(kind, 80)
    order = math.log2(e40 / e80)
    print("%s: error %.3e at T = 40, %.3e at T = 80, observed order %.2f" % (kind, e40, e80, order))
    assert order >= lo and (hi is None or order <= hi)


def test_a_table_without_its_history_term_is_first_order():
    """What the order test is for: DPM-Solver++(2M)'s rows with c dropped (and b left) no longer solve the ODE to second order."""
    from pww_hip import steps

    def error(T):
        sch = SC.make("dpmpp_2m", "epsilon", True, T)
        ts = sch.timesteps[:-1]
        sig = SC.sigmas_of(sch, ts)
        rows = steps.rows64(sch, ts)
        rows[:, 3] += rows[:, 4]          # first order: b = E, c = 0
        rows[:, 4] = 0.0
        x0 = SC.start("dpmpp_2m", sig[0])
        return SC.rel(SC.run_rows("dpmpp_2m", rows, sig, x0.clone(), "epsilon"), SC.exact_flow("dpmpp_2m", x0, sig[0], sig[-1]))
    assert math.log2(error(40) / error(80)) < 1.5


# ---- the classes: what the sampler's probes read

@pytest.mark.parametrize("kind, karras", [("euler", False), ("euler", True), ("euler_a", False), ("euler_a", True), ("ddim", False),
                                          ("dpmpp_2m", False), ("dpmpp_2m", True)])      # (DDIM has no use_karras_sigmas)
def test_scheduler_attributes_and_probes(kind, karras):
    from pww_hip.sampler import PwWSampler
    sch = SC.make(kind, "epsilon", karras, 5)
    assert len(sch) == 1000 and len(sch.timesteps) == 5 and tuple(sch.sigmas.shape) == (6,) and sch.sigmas.dtype == torch.float32 and float(sch.sigmas[-1]) == 0.0
    assert (sch.sigmas[:-1].diff() < 0).all() and sch.config.prediction_type == "epsilon" and sch.config.get("beta_schedule") == "scaled_linear"
    probe = SimpleProbe(sch)
    for i, t in enumerate(sch.timesteps):
        s = float(sch.sigmas[i])
        if kind in SC.SIGMA_SPACE:
            assert float(sch.init_noise_sigma) == float(sch.sigmas.max())
            assert PwWSampler._input_scale(probe, t, sch.sigmas[i]) == pytest.approx(math.sqrt(s * s + 1), rel=1e-6)
            assert PwWSampler._hold_coefficients(probe, t) == pytest.approx((1.0, s), rel=1e-6)
        else:
            assert float(sch.init_noise_sigma) == 1.0 and PwWSampler._input_scale(probe, t, sch.sigmas[i]) == 1.0
            a, b = PwWSampler._hold_coefficients(probe, t)
            assert b / a == pytest.approx(s, rel=1e-5) and a * a + b * b == pytest.approx(1.0, rel=1e-6)     # sigmas[i] IS sqrt((1 - abar) / abar)
    if kind in ("ddim", "dpmpp_2m") and not karras:
        assert sch.config.steps_offset == 1 and sch.timesteps.tolist() == [801, 601, 401, 201, 1]
        assert SC.make(kind, T=5, steps_offset=0).timesteps.tolist() == [800, 600, 400, 200, 0]
        ac = sch.alphas_cumprod[sch.timesteps]
        assert torch.allclose(sch.sigmas[:-1], ((1 - ac) / ac) ** 0.5, rtol=1e-6, atol=0)


class SimpleProbe:
    def __init__(self, scheduler):
        self.scheduler = scheduler


def test_a_stochastic_step_draws_exactly_one_randn(monkeypatch):
    calls = []
    real = torch.randn

    def randn(*args, **kw):
        calls.append((args, kw))
        return real(*args, **kw)
    monkeypatch.setattr(torch, "randn", randn)
    x = torch.ones(SC.SHAPE, dtype=torch.float32)
    for kind, want in (("euler", 0), ("euler_a", 1), ("ddim", 0), ("ddim_eta1", 1), ("dpmpp_2m", 0)):
        sch = SC.make(kind, T=3)
        del calls[:]
        for t in sch.timesteps:
            x = sch.step(torch.zeros_like(x), t, x).prev_sample
        assert len(calls) == 3 * want
        assert all(a == (x.shape,) and kw == dict(dtype=x.dtype, device=x.device) for a, kw in calls)


# ---- 3. covers and the keyword

def test_covers():
    from pww_hip import steps
    from sd_standin import LMSDiscreteScheduler, PLMSScheduler
    for kind in SC.KINDS:
        for prediction in SC.PREDICTIONS:
            assert steps.covers(SC.make(kind, prediction)) and steps.why_not(SC.make(kind, prediction)) is None
    assert not steps.covers(LMSDiscreteScheduler(**SC.BETAS)) and not steps.covers(PLMSScheduler()) and steps.why_not(PLMSScheduler()) == ""
    odd = SC.make("euler")
    odd.config["prediction_type"] = "sample"
    assert not steps.covers(odd) and "prediction_type" in steps.why_not(odd)
    for key, value in (("solver_order", 3), ("algorithm_type", "dpmsolver"), ("solver_type", "heun"), ("thresholding", True)):
        dpm = SC.make("dpmpp_2m")
        dpm.config[key] = value
        assert not steps.covers(dpm) and key in steps.why_not(dpm)

    class Renamed(type(SC.make("euler"))):
        pass
    assert not steps.covers(Renamed(**SC.BETAS)) and not steps.covers(object())
    with pytest.raises(ValueError, match="not covered"):
        steps.plan(PLMSScheduler(), [])
    # only the four names are routed at all: LMS and PLMS are not a decline, whatever PWW_STEP says
    steps.reset_stats()
    assert steps.route(PLMSScheduler(), torch.zeros(1)) is False and steps.stats()["declined"] == 0
    assert steps.stats() == {"requests": 0, "declined": 0, "fused_launches": 0, "decline_reasons": {}}


def test_the_switch(monkeypatch):
    from pww_hip import steps, _lib
    sch = SC.make("euler", T=2)
    steps.reset_stats()
    monkeypatch.setenv("PWW_STEP", "0")
    assert steps.route(sch, torch.zeros(1, dtype=torch.float64)) is False and steps.stats()["declined"] == 0
    monkeypatch.setenv("PWW_STEP", "1")
    assert steps.route(sch, torch.zeros(1, dtype=torch.float64)) is False
    assert steps.stats()["declined"] == 1 and list(steps.stats()["decline_reasons"]) == ["the latent is torch.float64, not float32"]
    monkeypatch.setenv("PWW_STEP", "force")
    with pytest.raises(_lib.PwwHipError, match="PWW_STEP=force: EulerDiscreteScheduler .* float32"):
        steps.route(sch, torch.zeros(1, dtype=torch.float64))
    monkeypatch.setenv("PWW_STEP", "yes")
    with pytest.raises(ValueError, match="PWW_STEP must be 0, 1 or force"):
        steps.route(sch, torch.zeros(1))
    monkeypatch.delenv("PWW_STEP")
    assert steps.mode(sch) == steps.DEFAULTS["EulerDiscreteScheduler"] and set(steps.DEFAULTS) == set(steps.NAMES)
    steps.reset_stats()
    assert "PWW_STEP" in open(REPO + "/INTEGRATION.md").read()


def test_keyword_position_and_default():
    import paint_with_words as pw
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    for f in (pw.paint_with_words, pw.paint_with_words_batch, inp.paint_with_words_inpaint, inp.paint_with_words_inpaint_batch):
        params = inspect.signature(f).parameters
        names = list(params)
        # (tests/test_region_prompts_host.py pins region_feather directly in front of max_prompt_chunks, the last keyword: `sampler` stands in
        # front of the region-prompt group, behind every keyword that was there before it)
        assert names[-5:] == ["sampler", "region_prompts", "region_base_weight", "region_feather", "max_prompt_chunks"]
        assert params["sampler"].default is None and "sampler" in f.__doc__
    doc = " ".join(pw.paint_with_words.__doc__.split())
    assert "steps_offset=0" in doc and "stays refused" in doc and all('"%s"' % name in doc for name in importlib.import_module("paint_with_words.paint_with_words").SAMPLERS)
    from pww_hip.sampler import PwWSampler
    assert "sampler" not in inspect.signature(PwWSampler.sample).parameters and "scheduler" not in inspect.signature(PwWSampler.sample).parameters
    from paint_with_words import pipelines
    for cls in (pipelines.PaintWithWord_StableDiffusionPipeline, pipelines.PaintWithWord_StableDiffusionInpaintPipeline):
        assert "sampler" not in inspect.signature(cls.__call__).parameters and not hasattr(cls, "sampler")


@pytest.mark.parametrize("bad", ["Euler", "heun", "", 3, ("euler",), True])
def test_a_bad_sampler_name_raises_before_the_tools_are_touched(rig, bad):      # noqa: F811
    class Untouchable(tuple):
        def __getitem__(self, i):
            raise AssertionError("the tools were touched")
    tools = Untouchable(_tools())
    calls = [lambda kw: rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, **kw),
             lambda kw: rig.pw.paint_with_words_batch(dict(CONTEXT), _color_map(), PROMPT, [0, 1], **kw),
             lambda kw: rig.inp.paint_with_words_inpaint(dict(CONTEXT), _color_map(), _mask(), _init_image(128), PROMPT, **kw),
             lambda kw: rig.inp.paint_with_words_inpaint_batch(dict(CONTEXT), _color_map(), _mask(), _init_image(128), PROMPT, [0], **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="sampler must be None or one of ddim, dpmpp_2m, dpmpp_2m_karras, euler, euler_a, euler_karras"):
            call(rig.kw(tools, sampler=bad))
    assert rig.events == [] and rig.encodes == []


def test_none_is_the_call_of_before_and_a_name_builds_a_scheduler_for_one_call(rig):      # noqa: F811
    tools = _tools()
    base = tools[4]
    plain = rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, seed=3, return_latents=True, **rig.kw(tools))
    a = rig.last()
    also = rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, seed=3, return_latents=True, **rig.kw(tools, sampler=None))
    b = rig.last()
    fake = [s for k, s in rig.events if k == "new"]
    assert len(fake) == 1 and not hasattr(fake[0], "scheduler")                 # None: the tools' scheduler, nothing swapped
    assert torch.equal(plain, also) and torch.equal(a.timesteps, b.timesteps) and torch.equal(a.timesteps, base.timesteps)
    seen = {}
    for name, (cls, kw) in rig.pw.SAMPLERS.items():
        real = fake[0].sample

        def sample(*args, _real=real, **kwargs):
            seen[name] = fake[0].scheduler
            return _real(*args, **kwargs)
        fake[0].sample = sample
        lat = rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, seed=3, return_latents=True, **rig.kw(tools, sampler=name))
        fake[0].sample = real
        sch, s = seen[name], rig.last()
        assert type(sch).__name__ == cls and fake[0].scheduler is base and tools[4] is base          # for this call only
        assert len([1 for k, _ in rig.events if k == "new"]) == 1                                   # the tools' sampler (and its graphs) serve every name
        assert (sch.config.beta_start, sch.config.beta_end, sch.config.prediction_type) == (0.00085, 0.012, "epsilon")
        assert bool(sch.config.get("use_karras_sigmas")) == bool(kw.get("use_karras_sigmas")) and torch.equal(s.timesteps, sch.timesteps)
        assert len(s.timesteps) == 3 and torch.allclose(lat, plain / base.init_noise_sigma * sch.init_noise_sigma, rtol=1e-6, atol=0)
    # the prediction type follows the tools' scheduler
    base.config["prediction_type"] = "v_prediction"
    fake[0].sample = lambda *a, **k: seen.__setitem__("v", fake[0].scheduler) or a[2]
    rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, return_latents=True, **rig.kw(tools, sampler="euler_a"))
    assert seen["v"].config.prediction_type == "v_prediction"


def test_region_strength_with_a_steps_offset_scheduler_stays_refused(rig):      # noqa: F811
    tools = _tools()
    for name in ("ddim", "dpmpp_2m", "dpmpp_2m_karras"):
        with pytest.raises(ValueError, match="steps_offset = 1"):
            rig.pw.paint_with_words(dict(CONTEXT), _color_map(), PROMPT, init_image=_init_image(64), region_strength={(0, 0, 0): 0.2},
                                    **rig.kw(tools, sampler=name))
    assert rig.events == [] and rig.encodes == []
    rig.pw._hold_scheduler_check(SC.make("dpmpp_2m", steps_offset=0))          # steps_offset=0 is accepted
    rig.pw._hold_scheduler_check(SC.make("ddim", steps_offset=0))
    rig.pw._hold_scheduler_check(SC.make("euler"))


# ---- 4. the table pair, the header, the exports, the refusals

def test_the_table_pair_holds_the_library(built_lib):
    import build as pww_build
    from pww_hip import _lib
    assert tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA)
    names = list(_lib.SIDE_EXTRA)
    assert names[-3:] == ["step", "control", "text"]
    spec = _lib.side_spec("step")
    assert spec is _lib.SIDE_EXTRA["step"] and set(spec) == set(_lib.SIDE["regions"]) and spec["missing_ok"] is True
    assert spec["exports"] is _lib.STEP_EXPORTS == ("pww_step_version", "pww_step_last_error", "pww_step_fwd") and spec["min_version"] == _lib.STEP_MIN_VERSION == 100
    assert spec["path"] == "STEP_LIB_PATH" and _lib.STEP_LIB_PATH.endswith("libpww_hip_step.so") and set(spec["sigs"]) == {"pww_step_fwd"}
    assert pww_build.SIDE_LIBS_EXTRA["step"][0] == "pww_step.hip" and pww_build.PER_FILE_FLAGS["pww_step.hip"] == ["-ffp-contract=off"]
    assert pww_build.LIB_STEP == pww_build.SIDE_PATHS["step"] and callable(pww_build.build_step) and callable(_lib.load_step)
    doc = pww_build.__doc__
    assert doc.index("Fifteen libraries") < doc.index("sixteenth") < doc.index("step      one sampler step")
    header = open(REPO + "/include/pww_hip_step.h").read()
    assert "#define PWW_STEP_VERSION 100" in header and "#define PWW_STEP_SRC_F32 2" in header and "#define PWW_STEP_ROW 7" in header
    assert (_lib.STEP_SRC_F32, _lib.STEP_ROW) == (2, 7)
    for fn in spec["exports"]:
        assert "%s(" % fn in header
    source = open(PKG + "/csrc/pww_step.hip").read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_step"' in source
    assert "atomic" not in source.replace("No atomics", "") and "__shared__" not in source
    assert "__fmaf" not in source and "fmaf(" not in source


@pytest.fixture(scope="module")
def step_lib(built_lib):
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_side("step")
    return _lib.load_side("step")


def test_a_real_load_binds_the_entry_points(step_lib):
    from pww_hip import _lib
    assert step_lib is not None and _lib.load_step() is step_lib and step_lib.pww_step_version() == 100
    for fn, (argtypes, restype) in _lib.SIDE_EXTRA["step"]["sigs"].items():
        assert getattr(step_lib, fn).argtypes == argtypes and getattr(step_lib, fn).restype is restype, fn
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.STEP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in dyn.splitlines() if " T " in line and not line.split()[-1].startswith(("_init", "_fini")))
    assert visible == sorted(_lib.STEP_EXPORTS)          # -fvisibility=hidden: the entry points and nothing else


def test_a_missing_file_is_not_an_error_but_a_decline(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "step", None)
    monkeypatch.setattr(_lib, "STEP_LIB_PATH", str(tmp_path / "libpww_hip_step.so"))
    assert _lib.load_step() is None


P, NULL = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)        # P is never dereferenced: validation precedes every launch
EINVAL, ENOTSUP = -22, -95
ROW = (1.0, -2.0, 0.5, 0.5, 0.0, 0.0, 1.5)


def _fwd(lib, x=P, h=NULL, m0=P, m1=P, g=7.5, z=NULL, u=NULL, row=ROW, n=256, copies=1, src=0, out=0):
    host = None if row is None else (ctypes.c_float * 7)(*row)
    return lib.pww_step_fwd(x, h, m0, m1, g, z, u, host, n, copies, src, out, None)


def _row(**kw):
    row = list(ROW)
    for k, v in kw.items():
        row["prabced".index(k)] = v
    return tuple(row)


REFUSALS = [
    (dict(x=NULL), EINVAL, "null"),                                        # a null latent
    (dict(m0=NULL), EINVAL, "null"),
    (dict(row=None), EINVAL, "null"),
    (dict(n=0), EINVAL, "0 elements"),                                     # n = 0
    (dict(n=-4), EINVAL, "-4 elements"),
    (dict(src=3), ENOTSUP, "unknown type 3"),                              # an unknown type
    (dict(src=-1), ENOTSUP, "unknown type -1"),
    (dict(u=P, out=2), ENOTSUP, "next input of unknown type 2"),
    (dict(m1=NULL), EINVAL, "m1 is required"),
    (dict(u=P, copies=0), EINVAL, "0 copies"),                             # u requested with copies < 1
    (dict(row=_row(c=0.25)), EINVAL, "needs the history h"),
    (dict(row=_row(e=0.25)), EINVAL, "needs the noise z"),
    (dict(row=_row(a=float("nan"))), EINVAL, "coefficient 2"),
    (dict(row=_row(d=float("inf"))), EINVAL, "coefficient 6"),
    (dict(g=float("nan")), EINVAL, "guidance scale"),
    (dict(u=P, row=_row(d=0.0)), EINVAL, "must be positive"),
    (dict(n=1 << 36), ENOTSUP, "2\\^36"),
]


def test_every_refusal_returns_before_a_hip_call_and_fills_the_error_slot(step_lib):
    import re
    from pww_hip import _lib
    seen = set()
    for kw, want, word in REFUSALS:
        rc = _fwd(step_lib, **kw)
        text = step_lib.pww_step_last_error().decode()
        assert rc == want, (kw, rc, text)
        assert text.startswith("step_fwd: ") and re.search(word, text), (kw, text)
        seen.add(text)
        with pytest.raises(_lib.PwwHipError) as e:
            _lib.check(rc, "pww_step_fwd", step_lib)
        assert text in str(e.value) and "rc=%d" % want in str(e.value)
    assert len(seen) >= 14                                   # each check has its own sentence


def test_ops_argument_checks():
    from pww_hip import ops
    from pww_hip._lib import PwwHipError
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.sched_step(x, ROW, torch.zeros_like(x))
