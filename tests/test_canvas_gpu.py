"""Canvases larger than the UNet's window on the GPU: the two launches of libpww_hip_canvas.so bit for bit against their restatements, one
folded UNet evaluation over the windows against the batch-1 calls, and whole loops in the three modes against the oracle canvas loop.

Expected values never come from the code under test: the gather is torch indexing, division and `.to(dtype)` on the CPU, the combine is the
header's formula in numpy fp32 (tests/canvas_cases.py), and the loop is tests/canvas_cases.py::oracle_canvas_loop -- per-window dicts from
the oracle's own encode_text_color_inputs on cropped maps, the numpy combine, the stand-in scheduler -- whose final latents are recorded in
tests/golden/canvas_oracle.npz (tests/test_canvas_host.py holds the record to fresh runs).

The fixture was measured on the CPU: on the 64 x 192 map the oracle's canvas result differs from the plain whole-canvas result of the same
seed by rel-L2 0.360 (profiles/canvas.md), against caps of 1e-2 (fp16) and 5e-2 (bf16)."""
import importlib
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import canvas_cases as C
import pww_cases as cases
from gpu_util import install_unfused, uninstall_all, rel_l2

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def _denoms():
    """1, and sqrt(sigma^2 + 1) in fp32 for the first and a late sigma of the 8-step LMS schedule."""
    sch = cases.build_tools("tiny")[4]
    sch.set_timesteps(C.STEPS)
    return [1.0] + [float((sch.sigmas[i] ** 2 + 1) ** 0.5) for i in (0, C.STEPS - 2)]


# ---- the two launches

@DTYPES
@pytest.mark.parametrize("case", list(C.KERNEL_CASES))
def test_gather_bit_for_bit(gpu_device, dtype, case):
    from pww_hip import ops
    (Hc, Wc), win, stride = C.KERNEL_CASES[case]
    ys, xs = C.grid(Hc, Wc, win, stride)
    assert tuple(ys) == ops.canvas_windows(Hc, win, stride) and tuple(xs) == ops.canvas_windows(Wc, win, stride)
    g = torch.Generator().manual_seed(ord(case))
    for C_ in ((4,) if case == "c" else (4, 5)):
        canvas = torch.randn(C_, Hc, Wc, generator=g) * 8.0
        canvas[0, 0, :4] = torch.tensor([0.0, 6e-8, 65000.0, -1e-5])                     # zero, an fp16 subnormal, near the fp16 maximum
        dev = canvas.to(gpu_device)
        for denom in ((_denoms()[1],) if case == "c" else _denoms()):                    # (c): the product shape, run once
            for copies in ((2,) if case == "c" else (1, 2, 5)):
                got = ops.canvas_gather(dev, ys, xs, win, win, denom, copies, dtype)
                want = C.gather(canvas, ys, xs, win, win, denom, copies, dtype)
                assert got.dtype == dtype and tuple(got.shape) == (copies * len(ys) * len(xs), C_, win, win)
                assert torch.equal(got.cpu(), want), (case, C_, denom, copies)
        assert torch.equal(ops.canvas_gather(dev[None], ys, xs, win, win, 1.0, 1, dtype), ops.canvas_gather(dev, ys, xs, win, win, 1.0, 1, dtype))


def _combine_inputs(case, K, C_, dtype, seed):
    (Hc, Wc), win, stride = C.KERNEL_CASES[case]
    ys, xs = C.grid(Hc, Wc, win, stride)
    n_w = len(ys) * len(xs)
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((K + 2) * n_w, C_, win, win, generator=g).to(dtype)
    more = {}
    if K:
        masks = torch.round(torch.rand(n_w, K, win, win, generator=g) * 64 / K) / 64     # multiples of 1 / 64 that sum to at most 1
        masks[:, :, 0, :3] = 0.0                                                         # ... with some zero spans
        masks[:, 0, 2:5, :] = 0.0
        weights = 0.05 + 0.9 * torch.rand(n_w, K, generator=g)
        scales = 1.0 + 14.0 * torch.rand(n_w, K, generator=g)
        assert len(set(weights.flatten().tolist())) == n_w * K and len(set(scales.flatten().tolist())) == n_w * K        # per window, all different
        more = dict(masks=masks, weights=weights, scales=scales)
    return ys, xs, (Hc, Wc), eps, more


@DTYPES
@pytest.mark.parametrize("case", list(C.KERNEL_CASES))
def test_combine_bit_for_bit(gpu_device, dtype, case):
    """K = 0, 1, 3 and ramp = 0, 1, 3, 4 at C = 4 (and 6 on the small cases: a second pass over the channels)."""
    from pww_hip import ops
    for K in ((3,) if case == "c" else (0, 1, 3)):
        for C_ in ((4,) if case in ("c", "d") else (4, 6)):
            ys, xs, hw, eps, more = _combine_inputs(case, K, C_, dtype, 100 * K + C_)
            dev = {k: v.to(gpu_device) for k, v in more.items()}
            outs = {}
            for ramp in ((4,) if case == "c" else (0, 1, 3, 4)):
                got = ops.canvas_combine(eps.to(gpu_device), ys, xs, hw, 7.5, ramp, **dev)
                want = C.combine(eps.float().numpy(), ys, xs, hw, 7.5, ramp, **{k: v.numpy() for k, v in more.items()})
                assert got.dtype == torch.float32 and tuple(got.shape) == (1, C_) + hw
                assert np.array_equal(got.cpu().numpy()[0], want), (case, K, C_, ramp)
                outs[ramp] = got
            if case != "c":
                assert torch.equal(outs[1], outs[0])                                     # ramp = 1 is ramp = 0, bit for bit
                if len(ys) * len(xs) > 1:
                    assert not torch.equal(outs[3], outs[0]) and not torch.equal(outs[4], outs[3])
            if case == "d" and K:
                # a single window with ramp = 0 is region_combine, bit for bit
                assert torch.equal(outs[0], ops.region_combine(eps.to(gpu_device), dev["masks"], dev["weights"], dev["scales"], 7.5))


# ---- one folded evaluation over the windows

@DTYPES
def test_one_folded_evaluation_matches_the_batch_1_calls(gpu_device, dtype):
    """Case (a) on the tiny UNet with 64-pixel windows, a 64 x 160 map: the rows of the folded call over the gathered windows (and of its
    hipGraph replay) against the batch-1 calls per window, inside the per-call attention bars taken at the UNet output: 2e-3 max|O| (fp16),
    1.6e-2 (bf16). Taken the way tests/test_region_prompts_gpu.py takes them: the UNet's weights are fp32, so what differs between the two
    sides is the attention path alone -- in fp16 by the package's cast of fp32 activations, in bf16 under torch.autocast. (A UNet whose every
    layer rounds to fp16 sits at 2.7e-3 max|O| between its own folded and batch-1 calls: the convolutions and norms of another batch size
    round differently, which is not what the attention bar is about.)"""
    import pww_hip
    from pww_hip import ops
    from pww_hip.conditioning import _encode_text_color_inputs
    from pww_hip.sampler import _fold_context, _GraphedUNet
    bar = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dtype]
    vae, unet, text, tok, sch = cases.build_tools("tiny", dtype=torch.float32, device=gpu_device, qk_gain=C.QK_GAIN)
    pww_hip.install(unet)
    try:
        rgb = C.color_map(64, 160)
        ys, xs = C.grid(8, 20, 8, 4)
        n_w = len(ys) * len(xs)
        pairs = [_encode_text_color_inputs(text, tok, gpu_device, crop, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "")[2:]
                 for crop in C.crops(rgb, ys, xs, 8, 8)]
        conds, unconds = [p[0] for p in pairs], [p[1] for p in pairs]
        canvas = (torch.randn(4, 8, 20, generator=torch.Generator().manual_seed(0)) * 3.0).to(gpu_device)
        sigma, t = torch.tensor(7.84), torch.tensor(888.0)
        x = ops.canvas_gather(canvas, ys, xs, 8, 8, float((sigma ** 2 + 1) ** 0.5), 2, dtype).float()
        wf, zero = cases.weight_fn_runner, (lambda w, sigma, qk: 0.0)
        with torch.no_grad(), warnings.catch_warnings(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            warnings.simplefilter("ignore")
            rows = []
            for dicts, f in ((conds, wf), (unconds, zero)):
                for j, d in enumerate(dicts):
                    d.update({"SIGMA": sigma, "WEIGHT_FUNCTION": f})
                    rows.append(unet(x[j:j + 1], t, encoder_hidden_states=d).sample)
            folded = _fold_context(conds, unconds, n_w, gpu_device)
            folded.update({"SIGMA": sigma, "WEIGHT_FUNCTION": wf})
            out_f = unet(x, t, encoder_hidden_states=folded).sample
            out_g = _GraphedUNet(unet)(0, x, 888.0, folded).clone()
        ref = torch.cat(rows).float()
        scale = ref.abs().max().item()
        err_f, err_g = (out_f.float() - ref).abs().max().item(), (out_g.float() - ref).abs().max().item()
        gaps = [(ref[j] - ref[0]).abs().max().item() for j in range(1, n_w)] + [(ref[n_w] - ref[0]).abs().max().item()]
        print("canvas fold check %s: folded %.3e, graph %.3e, max|eps| %.3f (bar %.3e), other windows / the unconditional row vs window 0 %s"
              % (dtype, err_f, err_g, scale, bar * scale, ["%.3e" % v for v in gaps]))
        assert tuple(out_f.shape) == (2 * n_w, 4, 8, 8)
        assert err_f <= bar * scale and err_g <= bar * scale
        assert min(gaps) > 4 * bar * scale                 # a row that landed on another window's place would show up as O(gap)
    finally:
        uninstall_all()


# ---- whole loops

def _set_mode(mode):
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    old, pww_mod.DEFAULT_MODE = pww_mod.DEFAULT_MODE, mode
    return pww_mod, old


def _hip_loop(tools, device, mode, name=None, fused=True, rgb=None, prompt=cases.RUNNER_PROMPT, steps=C.STEPS, canvas=True, stride=C.STRIDE, **kw):
    """paint_with_words on the map of loop `name` (or `rgb`), as a canvas request with the loop's ramp and region prompts -- or, canvas=False,
    as the plain call on the whole map."""
    import paint_with_words as pw
    from pww_hip import sampler as S
    ramp, regions = 0, None
    if name is not None:
        (H, W), ramp, regions = C.LOOPS[name]
        rgb = C.color_map(H, W)
    pww_mod, old = _set_mode(mode)
    orig_install = S.install
    if not fused:
        S.install = install_unfused        # calibration path: same driver, attention as unfused torch ops
    more = dict(canvas_window=C.WINDOW, canvas_stride=stride, canvas_ramp=ramp) if canvas else {}
    try:
        return pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=prompt,
                                   num_inference_steps=steps, guidance_scale=C.GUIDANCE, seed=C.SEED, device=str(device),
                                   weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True,
                                   region_prompts=None if regions is None or not canvas else dict(regions), **more, **kw).clone()
    finally:
        S.install = orig_install
        pww_mod.DEFAULT_MODE = old
        if not fused:
            uninstall_all()


@pytest.fixture(scope="module")
def oracle_latents():
    return C.recorded()


_UNFUSED = {}


def _unfused_drift(gpu_device, oracle_latents, dtype, name):
    """rel-L2 of the unfused torch path -- the same driver and the same two canvas launches, attention as torch ops in `dtype` -- against the
    oracle loop, once per (dtype, loop)."""
    if (dtype, name) not in _UNFUSED:
        tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=C.QK_GAIN)
        try:
            _UNFUSED[dtype, name] = rel_l2(_hip_loop(tools, gpu_device, "eager", name, fused=False), oracle_latents[name])
        finally:
            uninstall_all()
    return _UNFUSED[dtype, name]


@pytest.mark.parametrize("name", list(C.LOOPS))
@pytest.mark.parametrize("mode", ["eager", "folded", "graph"])
@DTYPES
def test_tiny_canvas_loop_vs_oracle(gpu_device, oracle_latents, dtype, mode, name):
    d0 = _unfused_drift(gpu_device, oracle_latents, dtype, name)
    tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=C.QK_GAIN)
    try:
        lat = _hip_loop(tools, gpu_device, mode, name)
    finally:
        uninstall_all()
    d = rel_l2(lat, oracle_latents[name])
    print(f"canvas loop {name} {dtype} {mode}: rel-L2 hip {d:.3e} unfused-torch {d0:.3e}")
    assert tuple(lat.shape) == tuple(oracle_latents[name].shape) and lat.dtype == torch.float32
    assert d <= C.CAP[dtype]
    assert d <= C.UNFUSED_SLACK[0] * d0 + C.UNFUSED_SLACK[1]


@DTYPES
def test_the_plain_call_lies_outside_the_cap(gpu_device, oracle_latents, dtype):
    """On the map the tiny UNet also takes as one image: the plain whole-canvas call lands on the plain oracle loop and far from the canvas
    loop's result -- the caps above would not pass a canvas path that denoised the whole canvas as one image."""
    tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=C.QK_GAIN)
    try:
        plain = _hip_loop(tools, gpu_device, "graph", C.PLAIN, canvas=False)
        same = _hip_loop(tools, gpu_device, "graph", C.PLAIN, canvas=False, canvas_window=C.LOOPS[C.PLAIN][0][1])      # a window as wide as the map: the plain call
    finally:
        uninstall_all()
    d_canvas, d_plain = rel_l2(plain, oracle_latents[C.PLAIN]), rel_l2(plain, oracle_latents["plain"])
    print(f"plain call {dtype}: vs the canvas oracle loop {d_canvas:.3e}, vs the plain oracle loop {d_plain:.3e}")
    assert d_canvas > 4 * max(C.CAP.values()) > C.CAP[dtype]
    assert d_plain <= {torch.float16: 2e-2, torch.bfloat16: 1e-1}[dtype]          # the plain loop's own caps (tests/test_loop_gpu.py)
    assert rel_l2(same, plain) <= 2e-2                                             # (two half-precision runs of one request: the loop cap of tests/test_loop_gpu.py)


# ---- hipGraph mode: one capture serves all steps and every request of the same window batch

def test_graph_captures(gpu_device):
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=C.QK_GAIN)
    steps = 4
    other_rgb = np.ascontiguousarray(np.roll(C.color_map(64, 160), 56, axis=1)[:, ::-1])       # another colour map of the same size ...
    # ... and another prompt. (Its last region phrase sits at position 20, the fixture's at 17: the same column bound of 32 -- the bound is
    # launch geometry, rounded up to 16 columns so that prompts like these replay one graph; pww_hip/conditioning.py.)
    other_prompt = "a photo of a tree and a cat, a happy dog running on wet ground under a cloudy sky"
    try:
        a = _hip_loop(tools, gpu_device, "graph", "a", steps=steps)
        sampler = tools[1]._pww_samplers[(id(tools[4]), "graph")]
        assert sampler._graphed.captures == 1 and len(sampler._graphed.graphs) == 1            # one capture for all steps
        b = _hip_loop(tools, gpu_device, "graph", rgb=other_rgb, prompt=other_prompt, steps=steps)
        assert sampler._graphed.captures == 1                                                  # replayed
        b_eager = _hip_loop(tools, gpu_device, "eager", rgb=other_rgb, prompt=other_prompt, steps=steps)
        assert rel_l2(b, b_eager) <= 2e-2 and rel_l2(a, b) > 4e-2                              # a stale map or embedding would show as O(1)
        # other origins of the same count: a 64 x 136 map has the windows 0, 4, 8, 9
        c = _hip_loop(tools, gpu_device, "graph", rgb=C.color_map(64, 136), steps=steps)
        assert sampler._graphed.captures == 1 and tuple(c.shape) == (1, 4, 8, 17)
        c_eager = _hip_loop(tools, gpu_device, "eager", rgb=C.color_map(64, 136), steps=steps)
        assert rel_l2(c, c_eager) <= 2e-2
        # another window count: captured again, once
        e = _hip_loop(tools, gpu_device, "graph", C.PLAIN, steps=steps)
        assert sampler._graphed.captures == 2 and tuple(e.shape) == (1, 4, 8, 24)
        a2 = _hip_loop(tools, gpu_device, "graph", "a", steps=steps)
        assert sampler._graphed.captures == 3 and rel_l2(a2, a) <= 2e-2
    finally:
        uninstall_all()


def test_record_attention_maps_is_refused(gpu_device):
    import pww_hip
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=C.QK_GAIN)
    try:
        for mode in ("eager", "graph"):
            with pww_hip.record_attention_maps():
                with pytest.raises(ValueError, match="record_attention_maps"):
                    _hip_loop(tools, gpu_device, mode, "a", steps=2)
        assert torch.isfinite(_hip_loop(tools, gpu_device, "graph", "a", steps=2)).all()        # and the next request runs
    finally:
        uninstall_all()
