"""The fused sampler step on the device: ops.sched_step against a torch-CPU fp32 restatement bit for bit; whole requests on the fused route
against the same requests on scheduler.step (PWW_STEP=0) in eager, folded and hipGraph mode; one captured graph for every scheduler; the
feature beside region prompts, a canvas, region strength, inpainting and a ControlNet. The tables themselves are tests/test_steps_host.py."""
import importlib

import pytest
import torch
from PIL import Image

import control_cases as CC
import hold_cases as H
import pww_cases as cases
import sched_cases as SC
from gpu_util import uninstall_all, rel_l2

pytestmark = pytest.mark.gpu

# The bar of the route tests: 4 x FLOOR. FLOOR is the largest rel-L2 between "eager" and "folded" mode of the STOCK route (PWW_STEP=0) over
# the cases of test_route_against_stock_route, measured on the MI355X -- two arithmetic-equivalent orders of the same computation that the
# tree already accepts; x 4 because the step's rounding enters T times and the UNet amplifies it. Taken per storage type (the float16 cases
# are held to the float16 floor, eight times lower; the largest value over all cases is the bfloat16 one). Measured: bfloat16 7.090e-02
# (euler_a, v_prediction), float16 9.692e-03 (euler_a, v_prediction); fused against stock: 8e-08 .. 1.2e-02 in bfloat16, 8e-08 .. 6.0e-03
# in float16 (profiles/schedulers.md, section 3).
FLOOR = {"bf16": 7.090e-02, "f16": 9.692e-03}
BAR = {dtype: 4 * floor for dtype, floor in FLOOR.items()}

HALF = {"f16": torch.float16, "bf16": torch.bfloat16}
SENTINEL = 12345.0


# ---- 5. the kernel, bit for bit

ROWS = {                                    # (p, r, a, b, c, e, d'): every (c, e) pair, and the last step of DPM-Solver++ (a = 0, b = 1)
    "plain": (1.0, -3.25, 0.625, 0.375, 0.0, 0.0, 3.4004),
    "history": (0.995, -1.7, 0.4143, 0.8811, -0.2957, 0.0, 1.0),
    "noise": (1.0, -14.6, 0.71, 0.29, 0.0, 2.3711, 10.391),
    "both": (0.08, -0.27, 0.31, 1.13, -0.21, 0.77, 1.0207),
    "last": (1.0, -0.0413, 0.0, 1.0, 0.0, 0.0, 1.0),
}
SHAPES = {"wide": ((1, 4, 8, 8), 1, 0), "ragged": ((1, 4, 5, 3), 1, 0), "copies3": ((3, 4, 8, 8), 3, 0), "offset1": ((1, 4, 8, 8), 1, 1)}


def _padded(values, device, offset, fill=SENTINEL):
    """`values` inside a longer device buffer of sentinels, `offset` elements from its (aligned) start -> (the buffer, the view)."""
    flat = values.reshape(-1)
    buf = torch.full((flat.numel() + offset + 16,), fill, dtype=values.dtype, device=device)
    buf[offset:offset + flat.numel()] = flat.to(device)
    return buf, buf[offset:offset + flat.numel()].view(values.shape)


def _untouched(buf, offset, numel, fill=SENTINEL):
    return bool((buf[:offset] == fill).all()) and bool((buf[offset + numel:] == fill).all())


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("src", ["f16", "bf16", "f32"])
def test_sched_step_bit_for_bit(gpu_device, src, shape):
    from pww_hip import ops
    dims, copies, offset = SHAPES[shape]
    out_dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.bfloat16}[src]
    g = torch.Generator().manual_seed(17)
    numel = int(torch.tensor(dims).prod())
    for name, row in ROWS.items():
        x, h, z = (torch.randn(dims, generator=g) * s for s in (3.0, 1.0, 1.0))
        if src == "f32":
            model, guidance = torch.randn(dims, generator=g), 0.0
        else:
            model, guidance = tuple(torch.randn(dims, generator=g).to(HALF[src]) for _ in range(2)), 7.5
        c, e = row[4], row[5]
        want_x, want_q, want_u = SC.step_reference(x, row, model, guidance, h, z, out_dtype, copies)
        # on the device: every tensor inside a longer buffer of sentinels; a term whose coefficient is 0 gets NaNs to read
        bx, dx = _padded(x, gpu_device, offset)
        bh, dh = _padded(h if c != 0.0 else torch.full(dims, float("nan")), gpu_device, offset)
        _, dz = _padded(z if e != 0.0 else torch.full(dims, float("nan")), gpu_device, offset)
        dm = tuple(_padded(m, gpu_device, offset)[1] for m in model) if src != "f32" else _padded(model, gpu_device, offset)[1]
        bu, du = _padded(torch.zeros((copies * dims[0],) + dims[1:], dtype=out_dtype), gpu_device, offset, fill=777.0)
        got = ops.sched_step(dx, row, dm, guidance, h=dh, z=dz, u=du)
        torch.cuda.synchronize()
        assert got is dx, name
        assert torch.equal(dx.cpu(), want_x) and torch.equal(dh.cpu(), want_q), (name, src, shape)
        assert torch.equal(du.cpu(), want_u), (name, src, shape)
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dh).all()) and bool(torch.isfinite(du.float()).all()), name
        rounded = (want_x / torch.tensor(row[6], dtype=torch.float32)).to(out_dtype)
        for k in range(copies):                                    # every replica is the single rounding of x' / d'
            assert torch.equal(du[k * dims[0]:(k + 1) * dims[0]].cpu(), rounded), (name, k)
        assert _untouched(bx, offset, numel) and _untouched(bh, offset, numel) and _untouched(bu, offset, copies * numel, 777.0), name
        if name == "last":
            assert torch.equal(dx, dh)                             # a = 0, b = 1: x' is q
        # no history, no noise, no next input: the pointers may be null
        if c == 0.0 and e == 0.0:
            _, alone = _padded(x, gpu_device, offset)
            ops.sched_step(alone, row, dm, guidance)
            assert torch.equal(alone.cpu(), want_x), name


def test_sched_step_checks_its_arguments(gpu_device):
    from pww_hip import ops
    from pww_hip._lib import PwwHipError
    x = torch.zeros(1, 4, 8, 8, device=gpu_device)
    m = torch.zeros_like(x)
    before = ops.STEP_LAUNCHES[0]
    with pytest.raises(PwwHipError, match="7 numbers"):
        ops.sched_step(x, ROWS["plain"][:6], m)
    with pytest.raises(PwwHipError, match="float32 x, h and z"):
        ops.sched_step(x, ROWS["plain"], m, h=torch.zeros(1, 4, 8, 4, device=gpu_device))
    with pytest.raises(PwwHipError, match="cond / uncond pair"):
        ops.sched_step(x, ROWS["plain"], (m.half(), m.bfloat16()))
    with pytest.raises(PwwHipError, match="single model output"):
        ops.sched_step(x, ROWS["plain"], m.half())
    with pytest.raises(PwwHipError, match=r"copies \* n"):
        ops.sched_step(x, ROWS["plain"], m, u=torch.zeros(2, 4, 8, 4, device=gpu_device, dtype=torch.float16))
    with pytest.raises(PwwHipError, match="contiguous"):
        ops.sched_step(x.permute(0, 1, 3, 2), ROWS["plain"], m)
    with pytest.raises(PwwHipError, match="needs the history h"):
        ops.sched_step(x, ROWS["history"], m)
    with pytest.raises(PwwHipError, match="needs the noise z"):
        ops.sched_step(x, ROWS["noise"], m)
    assert ops.STEP_LAUNCHES[0] == before and float(x.abs().max()) == 0.0


# ---- whole requests

RGB = CC.color_map(128)                     # 128 pixels: a latent of 16 x 16, 1024 elements -- several workgroups of the wide form


def _request(device, tools, mode, env, monkeypatch, steps=4, face=None, **kw):
    """One txt2img request of `steps` steps under PWW_STEP=env; the global generator (a stochastic scheduler's noise) seeded."""
    import paint_with_words as pw
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    monkeypatch.setenv("PWW_STEP", env)
    old, pww_mod.DEFAULT_MODE = pww_mod.DEFAULT_MODE, mode
    args = dict(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(RGB), input_prompt=cases.RUNNER_PROMPT)
    args.update(num_inference_steps=steps, guidance_scale=7.5, seed=0, device=str(device), weight_function=cases.weight_fn_runner, preloaded_utils=tools,
                return_latents=True)
    for key in kw.pop("drop", ()):          # (the batch faces name these arguments in the plural)
        args.pop(key)
    args.update(kw)
    try:
        torch.manual_seed(11)
        return (face or pw.paint_with_words)(**args).clone()
    finally:
        pww_mod.DEFAULT_MODE = old


def _pair(device, tools, mode, monkeypatch, **kw):
    """(fused, stock, launches of the fused request) of one request."""
    from pww_hip import steps
    steps.reset_stats()
    fused = _request(device, tools, mode, "force", monkeypatch, **kw)
    st = steps.stats()
    assert st["declined"] == 0 and st["requests"] == 1, st
    stock = _request(device, tools, mode, "0", monkeypatch, **kw)
    assert steps.stats()["fused_launches"] == st["fused_launches"]          # PWW_STEP=0: not one launch
    assert fused.dtype == torch.float32 and fused.shape == stock.shape and bool(torch.isfinite(fused).all())
    return fused, stock, st["fused_launches"]


# 6. per scheduler and prediction type, in the three modes, fused against stock
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("prediction", SC.PREDICTIONS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_route_against_stock_route(gpu_device, monkeypatch, kind, prediction, dtype):
    tools = cases.build_tools("tiny", dtype=HALF[dtype], device=gpu_device)[:4] + (SC.make(kind, prediction),)
    stock_setting = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        runs = {mode: _pair(gpu_device, tools, mode, monkeypatch) for mode in ("eager", "folded", "graph")}
    finally:
        torch.backends.cudnn.deterministic = stock_setting
        uninstall_all()
    floor = rel_l2(runs["folded"][1], runs["eager"][1])
    d = {mode: rel_l2(fused, stock) for mode, (fused, stock, _) in runs.items()}
    print("steps %s %s %s: stock eager vs stock folded %.3e; fused vs stock eager %.3e folded %.3e graph %.3e"
          % (kind, prediction, dtype, floor, d["eager"], d["folded"], d["graph"]))
    assert all(launches == 4 for _, _, launches in runs.values())            # ONE launch per step, in every mode
    for mode in runs:
        assert d[mode] <= BAR[dtype], (mode, d[mode])


# 7. one graph for every step and every scheduler
def test_one_graph_serves_every_scheduler(gpu_device, monkeypatch):
    from pww_hip import steps
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    try:
        steps.reset_stats()
        a = _request(gpu_device, tools, "graph", "force", monkeypatch, steps=4, sampler="euler")
        sampler = tools[1]._pww_samplers[(id(tools[4]), "graph")]
        assert sampler._graphed.captures == 1 and steps.stats()["fused_launches"] == 4
        b = _request(gpu_device, tools, "graph", "force", monkeypatch, steps=6, sampler="dpmpp_2m_karras")
        st = steps.stats()
        assert sampler._graphed.captures == 1 and len(sampler._graphed.graphs) == 1
        assert st["fused_launches"] == 4 + 6 and st["requests"] == 2 and st["declined"] == 0 and st["decline_reasons"] == {}
        assert sampler.scheduler is tools[4]                                   # the named scheduler served its call only
        c = _request(gpu_device, tools, "graph", "force", monkeypatch, steps=4)       # LMS, the tools' own: the route of before, same graph
        assert sampler._graphed.captures == 1 and steps.stats()["fused_launches"] == 10
        assert rel_l2(a, b) > 1e-2 and rel_l2(a, c) > 1e-3 and all(bool(torch.isfinite(t).all()) for t in (a, b, c))
    finally:
        uninstall_all()


# 8. composition: one small request each with sampler="dpmpp_2m", against PWW_STEP=0
def _compose(gpu_device, monkeypatch, tools, mode, launches_expected=4, **kw):
    """(the tools of these requests are float16)"""
    stock_setting = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        fused, stock, launches = _pair(gpu_device, tools, mode, monkeypatch, **kw)
    finally:
        torch.backends.cudnn.deterministic = stock_setting
        uninstall_all()
    d = rel_l2(fused, stock)
    print("steps composition %s: fused vs stock %.3e (%d launches)" % (sorted(set(kw) - {"sampler", "drop"}), d, launches))
    assert launches == launches_expected and d <= BAR["f16"]
    return fused


def test_with_region_prompts(gpu_device, monkeypatch):
    """The fp32 blend of ops.region_combine is handed in as m."""
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    colors = list(cases.RUNNER_CONTEXT)
    _compose(gpu_device, monkeypatch, tools, "graph", sampler="dpmpp_2m", region_prompts={colors[0]: "a dog on the sand", colors[1]: ("a cat", 0.8, 5.0)},
             region_feather=1.0)


def test_with_negative_regions_a_long_prompt_and_a_batch(gpu_device, monkeypatch):
    import paint_with_words as pw
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    colors = list(cases.RUNNER_CONTEXT)
    args = dict(drop=("color_context", "color_map_image", "input_prompt", "seed"), color_contexts=dict(cases.RUNNER_CONTEXT),
                color_map_images=Image.fromarray(RGB), input_prompts=cases.RUNNER_PROMPT + ", " + " ".join("word%d" % i for i in range(90)), seeds=[0, 1],
                max_prompt_chunks=2, negative_color_context={colors[0]: "blurry,1.0"}, unconditional_input_prompt="blurry, low quality", negative_strength=0.5)
    out = _compose(gpu_device, monkeypatch, tools, "folded", sampler="dpmpp_2m", face=pw.paint_with_words_batch, **args)
    assert tuple(out.shape) == (2, 4, 16, 16)


def test_with_a_lora_adapter(gpu_device, monkeypatch):
    import lora_cases as L
    from pww_hip import lora
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    lora.load_lora(tools[1], L.kohya_dict(L.adapter_factors(tools[1], "a")), "a")
    try:
        _compose(gpu_device, monkeypatch, tools, "graph", sampler="dpmpp_2m", lora=("a", 0.8))
    finally:
        lora.unload_lora(tools[1], "a")


def test_with_a_two_window_canvas(gpu_device, monkeypatch):
    """No u: the canvas gathers its own rows; the fp32 canvas-sized prediction of ops.canvas_combine is m."""
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    wide = Image.fromarray(RGB[32:96])                                        # 128 x 64 pixels: two 64-pixel windows side by side
    out = _compose(gpu_device, monkeypatch, tools, "graph", sampler="dpmpp_2m", color_map_image=wide, canvas_window=64, canvas_stride=64)
    assert tuple(out.shape) == (1, 4, 8, 16)


def test_img2img_with_region_strength_keeps_the_init_latent(gpu_device, monkeypatch):
    """A steps_offset=0 scheduler in the tools; ops.hold_apply changes x behind the step launch. The s = 0 half comes back as the encoded
    init latent, bit for bit, as tests/test_hold_gpu.py asserts for LMS."""
    from pww_hip import steps
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    rgb, init, region_strength, strength, sigma, _ = H.loop_inputs("half_keep")
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=H.QK_GAIN)[:4] + (SC.make("dpmpp_2m", steps_offset=0),)
    keep, real = {}, pww_mod._held_images

    def held(*a, **k):
        out = real(*a, **k)
        keep["init"] = out[2].clone()
        return out
    monkeypatch.setattr(pww_mod, "_held_images", held)
    kw = dict(color_map_image=Image.fromarray(rgb), init_image=Image.fromarray(init), strength=strength, region_strength=region_strength,
              region_strength_feather=sigma, steps=H.STEPS)
    stock_setting = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        fused, stock, launches = _pair(gpu_device, tools, "graph", monkeypatch, **kw)
    finally:
        torch.backends.cudnn.deterministic = stock_setting
        uninstall_all()
    d = rel_l2(fused, stock)
    print("steps composition region strength: fused vs stock %.3e (%d launches)" % (d, launches))
    assert 1 <= launches <= H.STEPS and d <= BAR["f16"]
    x0 = keep["init"]
    assert torch.equal(fused[..., :4], x0[..., :4]) and rel_l2(fused[..., 4:], x0[..., 4:]) > 0.1
    with pytest.raises(ValueError, match="steps_offset = 1"):
        _request(gpu_device, tools, "graph", "1", monkeypatch, sampler="dpmpp_2m", **kw)
    assert steps.stats()["declined"] == 0


def test_inpainting(gpu_device, monkeypatch):
    """No u: the input is the latent beside the mask and the masked image (`extra_channels`), made as before."""
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    tools = cases.build_tools("tiny_inpaint", dtype=torch.float16, device=gpu_device)
    mask = Image.fromarray((torch.arange(128)[:, None].expand(128, 128) < 64).numpy().astype("uint8") * 255)
    # (strength 1 with a steps_offset = 1 scheduler runs 3 of the 4 steps: the reference's img2img arithmetic)
    _compose(gpu_device, monkeypatch, tools, "graph", launches_expected=3, sampler="dpmpp_2m", face=inp.paint_with_words_inpaint, mask_image=mask,
             init_image=Image.fromarray(cases.synthetic_init_image(128)))


def test_with_a_controlnet(gpu_device, monkeypatch):
    tools, (net,) = CC.build_request_tools(gpu_device)
    _compose(gpu_device, monkeypatch, tools, "graph", sampler="dpmpp_2m", controlnet=net, control_image=CC.control_image(1))


def test_img2img_runs_a_suffix(gpu_device, monkeypatch):
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    init = Image.fromarray(cases.synthetic_init_image(128))
    for name in ("dpmpp_2m", "euler_a"):
        stock_setting = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            fused, stock, launches = _pair(gpu_device, tools, "folded", monkeypatch, sampler=name, init_image=init, strength=0.5, steps=6)
        finally:
            torch.backends.cudnn.deterministic = stock_setting
            uninstall_all()
        d = rel_l2(fused, stock)
        print("steps composition img2img %s: fused vs stock %.3e (%d launches)" % (name, d, launches))
        assert launches == 3 and d <= BAR["f16"]              # strength 0.5 of 6 steps
