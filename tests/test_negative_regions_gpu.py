"""Negative regions on the GPU: region-weighted attention on the unconditional rows of classifier-free guidance.

Expected values come from the oracle's building blocks, never from the code under test: `oracle.pww_oracle.encode_text_color_inputs` called
with (negative_color_context, unconditional prompt) gives the unconditional dict (its `cond`), and `oracle_loop` below is
`oracle.sample_latents` with the zero lambda of the unconditional pass replaced by `negative_strength * weight_function` -- the reference's
own `inj_forward` accepts exactly this dict.

The fixture (QK_GAIN, NEG_STRENGTH, NEG_CONTEXT) was picked on the CPU so that the feature is far above the parity bars: the oracle's final
latent with the negative context differs from the one without it by rel-L2 0.562 (profiles/negative_regions.md), against caps of 2e-2 (fp16)
and 1e-1 (bf16)."""
import importlib
import math

import numpy as np
import pytest
import torch
from PIL import Image

import pww_cases as cases
from gpu_util import TOL, install_unfused, uninstall_all, rel_l2
from oracle import pww_oracle as O

pytestmark = pytest.mark.gpu

from negative_cases import NEG_PROMPT, NEG_CONTEXT, NEG_STRENGTH, QK_GAIN, STEPS, CAP, oracle_loop      # noqa: E402  (the fixture, shared with the host tests)


def _set_mode(mode):
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    old, pww_mod.DEFAULT_MODE = pww_mod.DEFAULT_MODE, mode
    return pww_mod, old


def _hip_loop(tools, device, mode, neg_context, neg_strength=NEG_STRENGTH, steps=STEPS, seed=0, fused=True, wf=cases.weight_fn_runner, **kw):
    import paint_with_words as pw
    from pww_hip import sampler as S
    pww_mod, old = _set_mode(mode)
    orig_install = S.install
    if not fused:
        S.install = install_unfused        # calibration path: same driver, attention as unfused torch ops
    try:
        return pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()),
                                   input_prompt=cases.RUNNER_PROMPT, num_inference_steps=steps, guidance_scale=7.5, seed=seed, device=str(device),
                                   weight_function=wf, preloaded_utils=tools, return_latents=True, unconditional_input_prompt=NEG_PROMPT,
                                   negative_color_context=None if neg_context is None else dict(neg_context), negative_strength=neg_strength,
                                   **kw).clone()
    finally:
        S.install = orig_install
        pww_mod.DEFAULT_MODE = old
        if not fused:
            uninstall_all()


@pytest.fixture(scope="module")
def oracle_latents():
    return {"with": oracle_loop(NEG_CONTEXT, NEG_STRENGTH), "without": oracle_loop(None, 0.0)}


# ------------------------------------------------------------------------------------------------------------------------------------
# the weight maps of the negative table

def test_negative_weight_maps_are_the_oracles_bit_for_bit(gpu_device):
    from pww_hip.conditioning import _encode_text_color_inputs, PwWContext
    vae, unet, text, tok, sch = cases.build_tools("tiny", dtype=torch.float32, device=gpu_device)
    rgb = cases.load_example_rgb()
    neg = dict(NEG_CONTEXT)
    neg[(90, 206, 255)] = "low quality,0.7,-1"
    _, _, cond, uncond = _encode_text_color_inputs(text, tok, gpu_device, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, NEG_PROMPT,
                                                   negative_color_context=neg)
    assert neg[(90, 206, 255)] == "low quality,0.7" and isinstance(uncond, PwWContext)
    cpu_text = cases.build_tools("tiny")[2]
    want_neg = dict(NEG_CONTEXT)
    want_neg[(90, 206, 255)] = "low quality,0.7,-1"
    _, _, want, _ = O.encode_text_color_inputs(cpu_text, tok, rgb, want_neg, NEG_PROMPT, "")
    _, _, want_pos, _ = O.encode_text_color_inputs(cpu_text, tok, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, NEG_PROMPT)
    for n in (4096, 1024, 256, 64):
        key = "CROSS_ATTENTION_WEIGHT_%d" % n
        assert np.array_equal(uncond[key].cpu().numpy(), want[key].numpy()), key
        assert np.array_equal(cond[key].cpu().numpy(), want_pos[key].numpy()), key          # the positive side is untouched
        assert float(uncond[key].abs().sum()) > 0
    assert np.array_equal(uncond["CROSS_ATTENTION_WEIGHT_ORIG"].cpu().numpy(), want["CROSS_ATTENTION_WEIGHT_ORIG"].numpy())
    # a blurred negative region: pww_gauss_blur's bar (tests/test_mask_gpu.py: 2e-5)
    _, _, _, unc_b = _encode_text_color_inputs(text, tok, gpu_device, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, NEG_PROMPT,
                                               negative_color_context={(13, 255, 0): "tree,1.5,-1,6.0"})
    _, _, want_b, _ = O.encode_text_color_inputs(cpu_text, tok, rgb, {(13, 255, 0): "tree,1.5,-1,6.0"}, NEG_PROMPT, "")
    for n in (4096, 64):
        key = "CROSS_ATTENTION_WEIGHT_%d" % n
        assert np.abs(unc_b[key].cpu().numpy() - want_b[key].numpy()).max() <= 2e-5
    assert not np.array_equal(unc_b["CROSS_ATTENTION_WEIGHT_4096"].cpu().numpy(), uncond["CROSS_ATTENTION_WEIGHT_4096"].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------------------
# one folded cross-attention call, every row biased

KINDS = {"max": "STAT_MAX", "std": "STAT_STD", "none": "STAT_NONE"}
GATE = [1.0, 1.0, 0.5, 0.5]


def _reference_call(q, k, v, w, gate, kind, c0, H, scale):
    """fp32 CPU, image by image: oracle.attention_core with bias = c0 * stat_b(q k^T) * gate[b] * w[b]."""
    outs = []
    for b in range(q.shape[0]):
        qh, kh, vh = (O.split_heads(t[b:b + 1].float().cpu(), H) for t in (q, k, v))
        scores = torch.matmul(qh, kh.transpose(-1, -2))
        stat = {"max": scores.max(), "std": scores.std(), "none": torch.tensor(1.0)}[kind]
        bias = (c0 * stat * gate[b]) * w[b].float().cpu()
        outs.append(O.merge_heads(O.attention_core(qh, kh, vh, bias, scale)[0], H))
    return torch.cat(outs)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M", [77, 154, 231])
@pytest.mark.parametrize("shape", ["sd15_n4096", "sd15_n1024", "sd15_n256", "sd15_n64"])
def test_folded_call_with_every_row_biased(gpu_device, shape, M, dtype):
    """rows [cond, cond, uncond, uncond], a map of its own per row, gate [1, 1, 0.5, 0.5], hint 0, for qk.max() / qk.std() / no statistic:
    the lean / general launch of libpww_hip.so (77 keys) and the launches of libpww_hip_long.so (154 / 231), with the statistic's partials
    from pww_qk_parts / pww_long_qk_parts and, where the product takes that route, from the to_q GEMM's epilogue (pww_qproj_stat)."""
    from pww_hip import ops, attention
    dev = gpu_device
    N, C, H, _ = cases.ATTN_SHAPES[shape]
    D, B = C // H, 4
    g = torch.Generator().manual_seed(N + M)
    x = (torch.randn(B, N, C, generator=g) * 0.5).to(dev, dtype)
    wq = (torch.randn(C, C, generator=g) * (2.0 / math.sqrt(C))).to(dev, dtype)
    k = torch.randn(B, M, C, generator=g).to(dev, dtype)
    v = torch.randn(B, M, C, generator=g).to(dev, dtype)
    cols = {77: 30, 154: 100, 231: 150}[M]                          # columns that carry weight; the bound is rounded up to 16
    w = (torch.rand(B, 1, N, M, generator=g) < 0.2).float() * torch.rand(B, 1, N, M, generator=g) * 1.5
    w[..., cols:] = 0.0
    assert not torch.equal(w[0], w[2]) and not torch.equal(w[2], w[3])
    wd = w.to(dev)
    bias_cols = (cols + 15) // 16 * 16
    gate = torch.tensor(GATE, device=dev)
    scale = D ** -0.5
    # a scalar per statistic, so that the bias is a few raw-score standard deviations in each case (max ~ 5 sigma, std = sigma, none = 1)
    c0s = {"max": 0.37, "std": 2.0, "none": 12.0}
    q_gemm = torch.nn.functional.linear(x, wq)
    routes = [("qk_parts", False)]
    if M <= ops.FUSED_MAX_KEYS and attention.qproj_route(C, D) and ops.qproj_parts(x, wq, k, H) > 0:
        routes.append(("qproj_stat", True))
    assert shape != "sd15_n4096" or M != 77 or len(routes) == 2     # the C = 320 layers do take the GEMM-epilogue route
    for kind in ("max", "std", "none"):
        code, c0 = getattr(ops, KINDS[kind]), c0s[kind]
        for name, qproj in routes:
            if qproj and kind == "none":
                continue            # (no statistic: nothing for the epilogue to form -- the plug takes the stock GEMM)
            if qproj:
                q, parts = ops.qproj_stat(x, wq, k, H, code, gate=gate)
            else:
                q = q_gemm
                parts = None
                if kind != "none":
                    parts = (ops.qk_parts if M <= ops.FUSED_MAX_KEYS else ops.long_qk_parts)(q, k, H, code, gate=gate, gated=0)
            out = ops.attention(q, k, v, H, scale, bias=wd, bias_coeff=gate, stat=(None, code, c0), parts=parts, bias_cols=bias_cols, gated=0)
            torch.cuda.synchronize()
            ref = _reference_call(q, k, v, w, GATE, kind, c0, H, scale)
            err = (out.float().cpu() - ref).abs().max().item()
            bar = TOL[dtype] * ref.abs().max().item()
            # the feature is in the output: the same call with the unconditional rows gated out differs on exactly those rows
            off = ops.attention(q, k, v, H, scale, bias=wd, bias_coeff=torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev), stat=(None, code, c0),
                                parts=parts, bias_cols=bias_cols, gated=0)
            moved = (out[2:].float() - off[2:].float()).abs().max().item()
            print("%s M=%d %s %s %s: max err %.3e (bar %.3e), uncond rows moved by %.3e" % (shape, M, str(dtype)[6:], kind, name, err, bar, moved))
            assert err <= bar, (kind, name, err, bar)
            assert torch.equal(out[:2], off[:2]) and moved > 4 * bar


def test_unconditional_rows_attend_to_the_negative_phrase(gpu_device):
    """Direction: with the negative map, the unconditional row puts MORE probability on the phrase's columns, summed over the region's
    queries, than without it (guidance then pushes away from that)."""
    from pww_hip import ops
    dev, dtype = gpu_device, torch.float16
    N, C, H, _ = cases.ATTN_SHAPES["sd15_n1024"]
    g = torch.Generator().manual_seed(5)
    q = (torch.randn(2, N, C, generator=g) * 0.5).to(dev, dtype)
    k = torch.randn(2, 77, C, generator=g).to(dev, dtype)
    region, cols = slice(0, N // 4), [3, 4]
    w = torch.zeros(2, 1, N, 77)
    w[1, 0, region, 3:5] = 1.0                                         # the negative phrase's columns inside its region, unconditional row only
    gate = torch.tensor([1.0, NEG_STRENGTH], device=dev)
    stats = ops.qk_stats(q, k, H)
    c0 = 0.4 * math.log(1 + 7.84)
    on = ops.attention_probs(q, k, H, (C // H) ** -0.5, bias=w.to(dev), bias_coeff=gate, stat=(stats, ops.STAT_MAX, c0))
    off = ops.attention_probs(q, k, H, (C // H) ** -0.5)
    mass_on, mass_off = on[1, region][:, cols].sum().item(), off[1, region][:, cols].sum().item()
    print("unconditional row, mass on the negative phrase inside the region: %.3f with the map, %.3f without" % (mass_on, mass_off))
    assert mass_on > 1.5 * mass_off
    torch.testing.assert_close(on[0], off[0], rtol=1e-4, atol=1e-5)     # the conditional row's map is all zero here: unchanged


# ------------------------------------------------------------------------------------------------------------------------------------
# loops

@pytest.mark.parametrize("mode", ["eager", "folded", "graph"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_tiny_loop_with_negative_regions_vs_oracle(gpu_device, oracle_latents, dtype, mode):
    tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=QK_GAIN)
    try:
        lat = _hip_loop(tools, gpu_device, mode, NEG_CONTEXT)
        plain = _hip_loop(tools, gpu_device, mode, None)
        base = _hip_loop(cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=QK_GAIN), gpu_device, "eager", NEG_CONTEXT, fused=False)
    finally:
        uninstall_all()
    d, d0 = rel_l2(lat, oracle_latents["with"]), rel_l2(base, oracle_latents["with"])
    d_plain = rel_l2(plain, oracle_latents["without"])
    visible = rel_l2(lat, plain)
    print(f"negative regions tiny {dtype} {mode}: rel-L2 hip {d:.3e} unfused-torch {d0:.3e}; without negatives {d_plain:.3e}; with vs without {visible:.3e}")
    assert d <= 1.5 * d0 + 2e-3
    assert d <= CAP[dtype]
    assert d_plain <= CAP[dtype]                       # None takes today's path, with this unconditional prompt too
    assert visible >= 2 * CAP[dtype]                   # the feature is far above the bar it is checked at


def test_folded_and_graph_match_eager_single_forward_with_negatives(gpu_device):
    """tests/test_loop_gpu.py::test_folded_and_graph_match_eager_single_forward with the unconditional rows biased: one fp32 UNet evaluation,
    [cond; uncond] folded (gate [1, 1, s, s], a map per row class, per-image statistic) and its hipGraph replay against the four batch-1 calls."""
    import warnings
    import pww_hip
    from pww_hip.conditioning import _encode_text_color_inputs
    from pww_hip.sampler import _fold_context, _GraphedUNet
    vae, unet, text, tok, sch = cases.build_tools("tiny", dtype=torch.float32, device=gpu_device, qk_gain=QK_GAIN)
    pww_hip.install(unet)
    try:
        _, _, cond, uncond = _encode_text_color_inputs(text, tok, gpu_device, cases.load_example_rgb(), dict(cases.RUNNER_CONTEXT),
                                                       cases.RUNNER_PROMPT, NEG_PROMPT, negative_color_context=dict(NEG_CONTEXT))
        _, _, _, uncond0 = _encode_text_color_inputs(text, tok, gpu_device, cases.load_example_rgb(), dict(cases.RUNNER_CONTEXT),
                                                     cases.RUNNER_PROMPT, NEG_PROMPT)
        x = torch.randn(2, 4, 64, 64, generator=torch.Generator().manual_seed(0)).to(gpu_device)
        sigma, t = torch.tensor(7.84), torch.tensor(888.0)
        wf = cases.weight_fn_runner
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cond.update({"SIGMA": sigma, "WEIGHT_FUNCTION": wf})
            uncond.update({"SIGMA": sigma, "WEIGHT_FUNCTION": lambda w, sigma, qk: NEG_STRENGTH * wf(w, sigma, qk)})
            uncond0.update({"SIGMA": sigma, "WEIGHT_FUNCTION": lambda w, sigma, qk: 0.0})
            e_c = torch.cat([unet(x[i:i + 1], t, encoder_hidden_states=cond).sample for i in range(2)])
            e_u = torch.cat([unet(x[i:i + 1], t, encoder_hidden_states=uncond).sample for i in range(2)])
            e_u0 = torch.cat([unet(x[i:i + 1], t, encoder_hidden_states=uncond0).sample for i in range(2)])
            folded = _fold_context(cond, uncond, 2, gpu_device, negative_strength=NEG_STRENGTH)
            folded.update({"SIGMA": sigma, "WEIGHT_FUNCTION": wf})
            out_f = unet(torch.cat([x, x]), t, encoder_hidden_states=folded).sample
            out_g = _GraphedUNet(unet)(0, torch.cat([x, x]), 888.0, folded).clone()
        ref = torch.cat([e_c, e_u]).float()
        scale = ref.abs().max().item()
        err_f = (out_f.float() - ref).abs().max().item()
        err_g = (out_g.float() - ref).abs().max().item()
        gap = (e_u.float() - e_u0.float()).abs().max().item()
        print(f"fold check with negatives: folded {err_f:.3e}, graph {err_g:.3e}, max|eps| {scale:.3f}, uncond with-vs-without gap {gap:.3e}")
        assert err_f <= 2e-3 * scale and err_g <= 2e-3 * scale
        assert gap > 20 * max(err_f, err_g)          # the negative bias matters: a gating bug would show up as O(gap)
    finally:
        uninstall_all()


def test_batch_with_per_image_negative_contexts_matches_single_calls(gpu_device):
    """Image i of paint_with_words_batch with one negative context per seed (one of them None) is the single-image call on request i."""
    import paint_with_words as pw
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=QK_GAIN)
    img = Image.fromarray(cases.load_example_rgb())
    negs = [dict(NEG_CONTEXT), {(255, 255, 255): "dog,2.0"}, None]
    seeds = [5, 6, 7]
    kw = dict(num_inference_steps=8, guidance_scale=7.5, device=str(gpu_device), weight_function=cases.weight_fn_runner, preloaded_utils=tools,
              return_latents=True, unconditional_input_prompt=NEG_PROMPT, negative_strength=NEG_STRENGTH)
    try:
        pww_mod, old = _set_mode("eager")
        try:
            single = torch.cat([pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=img, input_prompt=cases.RUNNER_PROMPT,
                                                    seed=s, negative_color_context=None if n is None else dict(n), **kw).clone()
                                for s, n in zip(seeds, negs)])
            pww_mod.DEFAULT_MODE = "graph"
            batched = pw.paint_with_words_batch(dict(cases.RUNNER_CONTEXT), img, cases.RUNNER_PROMPT, seeds,
                                                negative_color_context=[None if n is None else dict(n) for n in negs], **kw).clone()
            no_neg = pw.paint_with_words_batch(dict(cases.RUNNER_CONTEXT), img, cases.RUNNER_PROMPT, seeds, **kw).clone()
        finally:
            pww_mod.DEFAULT_MODE = old
    finally:
        uninstall_all()
    d_batch = rel_l2(batched, single)
    print("per-image negative contexts, 3-image graph batch vs one-by-one eager: %.3e; image 2 (no context) vs the batch without negatives %.3e; "
          "image 0 with vs without %.3e" % (d_batch, rel_l2(batched[2:], no_neg[2:]), rel_l2(batched[:1], no_neg[:1])))
    assert d_batch <= 1e-2
    assert rel_l2(batched[2:], no_neg[2:]) <= 1e-2 and rel_l2(batched[:1], no_neg[:1]) >= 2 * CAP[torch.float16]


def test_inpaint_loop_and_pipeline_class_run_with_a_negative_context(gpu_device):
    import paint_with_words as pw
    try:
        tools = cases.build_tools("tiny_inpaint", dtype=torch.float16, device=gpu_device)
        neg = {(136, 178, 92): "full moon,1.5,-1,4.0"}
        kw = dict(color_map_image=Image.fromarray(cases.load_aurora_rgb()), mask_image=cases.load_moon_mask(), init_image=Image.fromarray(cases.synthetic_init_image()),
                  input_prompt=cases.AURORA_PROMPT, num_inference_steps=4, guidance_scale=7.5, seed=81, device=str(gpu_device),
                  weight_function=cases.weight_fn_inpaint, preloaded_utils=tools, strength=1.0, return_latents=True,
                  unconditional_input_prompt="a full moon, blurry")
        with_neg = pw.paint_with_words_inpaint(color_context=dict(cases.INPAINT_CONTEXT), negative_color_context=neg, negative_strength=2.0, **kw).clone()
        without = pw.paint_with_words_inpaint(color_context=dict(cases.INPAINT_CONTEXT), **kw).clone()
        assert neg == {(136, 178, 92): "full moon,1.5"}                                       # stripped like color_context
        assert torch.isfinite(with_neg).all() and rel_l2(with_neg, without) > 1e-2
        both = pw.paint_with_words_inpaint_batch(dict(cases.INPAINT_CONTEXT), kw["color_map_image"], kw["mask_image"], kw["init_image"], cases.AURORA_PROMPT, [81, 81],
                                                 negative_color_context=[{(136, 178, 92): "full moon,1.5,-1,4.0"}, None], negative_strength=2.0,
                                                 **{k: v for k, v in kw.items() if k not in ("color_map_image", "mask_image", "init_image", "input_prompt", "seed")})
        # (image i of the batch is request i: the fp16 loop cap of tests/test_loop_gpu.py between two half-precision runs of one request)
        assert rel_l2(both[:1], with_neg) <= 2e-2 and rel_l2(both[1:], without) <= 2e-2
        uninstall_all()
        # the pipeline class: attributes, the call signature is the reference's
        vae, unet, text, tok, sch = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=QK_GAIN)
        pipe = pw.PaintWithWord_StableDiffusionPipeline(vae, text, tok, unet, sch)
        call = dict(prompt=cases.RUNNER_PROMPT, color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()),
                    num_inference_steps=3, guidance_scale=7.5, weight_function=cases.weight_fn_runner, negative_prompt=NEG_PROMPT, output_type="np")
        plain = pipe(**call).images[0]
        pipe.negative_color_context, pipe.negative_strength = dict(NEG_CONTEXT), NEG_STRENGTH
        painted = pipe(**call).images[0]
        assert plain.shape == painted.shape == (512, 512, 3) and np.isfinite(painted).all()
        assert np.abs(painted - plain).mean() > 1e-3
    finally:
        uninstall_all()


# ------------------------------------------------------------------------------------------------------------------------------------
# hipGraph capture count and the attention-map recorder

def test_graph_captures_and_recorder_with_negatives(gpu_device):
    import pww_hip
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=QK_GAIN)
    other = {(13, 255, 0): "tree,0.5", (255, 255, 255): "dog,2.5", (0, 0, 0): "cat,0.3", (90, 206, 255): "sky,2.0", (74, 18, 1): "ground,0.1"}    # same geometry (same phrases, same column bound), other maps
    steps = 4
    try:
        a = _hip_loop(tools, gpu_device, "graph", NEG_CONTEXT, steps=steps, seed=1)
        sampler = tools[1]._pww_samplers[(id(tools[4]), "graph")]
        assert sampler._graphed.captures == 1 and len(sampler._graphed.graphs) == 1
        b = _hip_loop(tools, gpu_device, "graph", other, neg_strength=0.75, steps=steps, seed=1)
        assert sampler._graphed.captures == 1                               # another negative map and strength: replayed
        b_folded = _hip_loop(tools, gpu_device, "folded", other, neg_strength=0.75, steps=steps, seed=1)
        assert rel_l2(b, b_folded) <= 2e-2 and rel_l2(a, b) > 2e-2          # a stale map or gate would show as O(1)
        off = _hip_loop(tools, gpu_device, "graph", None, steps=steps, seed=1)
        assert sampler._graphed.captures == 2                               # negatives off: captured again, once
        off2 = _hip_loop(tools, gpu_device, "graph", {}, steps=steps, seed=2)
        assert sampler._graphed.captures == 2 and rel_l2(off, a) > 2e-2 and torch.isfinite(off2).all()
        a2 = _hip_loop(tools, gpu_device, "graph", NEG_CONTEXT, steps=steps, seed=1)
        assert sampler._graphed.captures == 3 and rel_l2(a2, a) <= 2e-2
        # the recorder: n = 1 image, the conditional rows, in graph mode as in eager mode
        maps = {}
        for mode in ("eager", "graph"):
            with pww_hip.record_attention_maps() as rec:
                lat = _hip_loop(tools, gpu_device, mode, NEG_CONTEXT, steps=steps, seed=1)
            maps[mode] = rec.maps()
            if mode == "graph":
                assert torch.equal(lat, a2)                                  # recording changes no latent bit
        n_cross = sum(1 for name, _ in tools[1].named_modules() if name.endswith("attn2"))
        assert maps["graph"].counts == maps["eager"].counts and sum(maps["graph"].counts.values()) == n_cross * steps
        for N in maps["graph"].resolutions:
            got, want = maps["graph"].raw(N), maps["eager"].raw(N)
            assert got.shape[0] == 1 and got.shape == want.shape
            d = rel_l2(got, want)
            print("N = %d: graph (negatives on) vs eager conditional-row maps rel-L2 %.3e" % (N, d))
            assert d <= 1e-2
    finally:
        uninstall_all()
