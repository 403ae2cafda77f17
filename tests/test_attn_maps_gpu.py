"""Attention-map recording on the GPU: pww_cross_attn_probs against an fp64 restatement, its exact properties, the coefficient
through the plug, and whole sampling loops with the recorder on.

Bar of the numerical comparisons: max abs error <= 4 x the max abs error of the SAME formula evaluated by torch in fp32 on the GPU
(against fp64), + 1e-6. The factor covers the MFMA's summation order and the hardware exp; the yardstick is torch's fp32 error,
never the kernel's own."""
import importlib
import math

import numpy as np
import pytest
import torch
from PIL import Image

import pww_cases as cases
from gpu_util import uninstall_all, rel_l2

pytestmark = pytest.mark.gpu


def _ref(q, k, H, scale, bias, c, dt):
    """weight-free formula of the issue on the rounded q / k: mean_h softmax_m((Q K^T + c[b] bias) scale), in dtype dt."""
    B, N, C = q.shape
    M, D = k.shape[1], C // H
    qh = q.to(dt).reshape(B, N, H, D).permute(0, 2, 1, 3)
    kh = k.to(dt).reshape(k.shape[0], M, H, D).permute(0, 2, 3, 1)
    s = qh @ kh
    if bias is not None:
        s = s + c.to(dt).reshape(-1, 1, 1, 1) * bias.to(dt)
    return (s * scale).softmax(-1).mean(1)


def _stat_value(st, kind, count):
    from pww_hip import ops
    st = st.double()
    if kind == ops.STAT_MAX:
        return st[:, 0]
    if kind == ops.STAT_STD:
        return ((st[:, 3] - st[:, 2] ** 2 / count) / (count - 1)).clamp_min(0).sqrt()
    return torch.ones_like(st[:, 0])


def _check(name, got, q, k, H, scale, bias, c, weight=1.0, base=None):
    r64 = _ref(q, k, H, scale, bias, c, torch.float64)[:got.shape[0]] * weight
    r32 = _ref(q, k, H, scale, bias, c, torch.float32)[:got.shape[0]].double() * weight
    if base is not None:
        r64, r32 = r64 + base.double(), r32 + base.double()
    err, yard = (got.double() - r64).abs().max().item(), (r32 - r64).abs().max().item()
    print("%s: max abs err %.3e, fp32 torch %.3e, ratio %.2f" % (name, err, yard, err / max(yard, 1e-30)))
    assert err <= 4 * yard + 1e-6, (name, err, yard)


# (H, N, D): the four SD1.5 levels, SD2.x, two ragged token counts
SHAPES = [(8, 4096, 40), (8, 1024, 80), (8, 256, 160), (8, 64, 160), (5, 1024, 64), (8, 4000, 40), (8, 100, 40)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_probs_kernel_vs_fp64(gpu_device, dtype):
    from pww_hip import ops
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(7)
    case = 0
    for (H, N, D) in SHAPES:
        big = N >= 4000
        for M in ((77,) if big else (77, 64, 128)):
            for std in ((1.0,) if big and dtype == torch.bfloat16 else (1.0, 4.0)):
                case += 1
                B, scale = 3, D ** -0.5
                # scaled logits q.k * scale of standard deviation `std`: var(q.k) = D * vq * vk
                amp = math.sqrt(std)
                q = (torch.randn(B, N, H * D, generator=g) * amp).to(dev, dtype)
                k = (torch.randn(B, M, H * D, generator=g) * amp).to(dev, dtype)
                w = ((torch.rand(N, M, generator=g) < 0.15).float() * torch.rand(N, M, generator=g) * 1.5).to(dev)
                gate = torch.tensor([1.0, 0.0, 1.0], device=dev)
                tag = "H%d N%d D%d M%d %s std%g" % (H, N, D, M, str(dtype)[6:], std)
                count = float(H * N * M)
                # no map
                _check(tag + " plain", ops.attention_probs(q, k, H, scale), q, k, H, scale, None, None)
                # map with a per-image coefficient vector that holds a zero ("plain" route of ops.attention)
                cvec = torch.tensor([0.8, 0.0, -0.3], device=dev)
                _check(tag + " map", ops.attention_probs(q, k, H, scale, bias=w, bias_coeff=cvec), q, k, H, scale, w, cvec)
                # statistic formed in the kernel, times the gate; images < B
                st = ops.qk_stats(q, k, H)
                kind = (ops.STAT_MAX, ops.STAT_STD, ops.STAT_NONE)[case % 3]
                scalar = 0.4 * math.log(1 + 7.84) if kind != ops.STAT_STD else 0.9
                c = (torch.tensor(scalar, dtype=torch.float32, device=dev) * _stat_value(st, kind, count).float()) * gate
                got = ops.attention_probs(q, k, H, scale, bias=w, bias_coeff=gate, stat=(st if kind != ops.STAT_NONE else None, kind, scalar), images=2)
                assert tuple(got.shape) == (2, N, M)
                _check(tag + " stat%d" % kind, got, q, k, H, scale, w, c)
                if case % 2 == 0:
                    continue
                # accumulate on a pre-filled buffer with weight 0.25 and a padded row stride
                store = torch.full((B, N, 136), 7.0, device=dev)
                base = torch.rand(B, N, M, generator=g).to(dev)
                out = store[:, :, :M]
                out.copy_(base)
                ops.attention_probs(q, k, H, scale, bias=w, bias_coeff=cvec, out=out, accumulate=True, weight=0.25)
                _check(tag + " accumulate", out, q, k, H, scale, w, cvec, weight=0.25, base=base)
                assert bool((store[:, :, M:] == 7.0).all())


def test_probs_exact_properties(gpu_device):
    from pww_hip import ops
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(11)
    for (H, N, D, M, dtype) in [(8, 1000, 40, 77, torch.float16), (5, 256, 64, 128, torch.bfloat16), (8, 64, 160, 64, torch.float16)]:
        B, scale = 3, D ** -0.5
        q = (torch.randn(B, N, H * D, generator=g) * 1.5).to(dev, dtype)
        k = (torch.randn(B, M, H * D, generator=g) * 1.5).to(dev, dtype)
        w = torch.rand(N, M, generator=g).to(dev)
        cvec = torch.tensor([2.0, 0.5, 1.0], device=dev)
        for weight in (1.0, 0.25):
            poison = 1234.5
            store = torch.full((B, N, 132), poison, device=dev)
            out = store[:, :, :M]
            ops.attention_probs(q, k, H, scale, bias=w, bias_coeff=cvec, images=2, out=out, weight=weight)
            sums = out[:2].sum(-1)
            print("H%d N%d D%d M%d: max |row sum - weight| = %.3e" % (H, N, D, M, (sums - weight).abs().max().item()))
            assert (sums - weight).abs().max().item() <= 1e-5           # <= 128 fp32 terms, each good to a few ulp
            assert bool((out[:2] >= 0).all())
            assert bool((store[2] == poison).all())                      # images >= `images` are untouched
            assert bool((store[:, :, M:] == poison).all())               # so are the padding columns of a strided `out`
            again = torch.full((B, N, 132), poison, device=dev)
            ops.attention_probs(q, k, H, scale, bias=w, bias_coeff=cvec, images=2, out=again[:, :, :M], weight=weight)
            assert torch.equal(store, again)                             # two identical calls: identical bits


@pytest.mark.parametrize("route,shape", [("qproj", "sd15_n4096"), ("qk_parts", "sd15_n256"), ("plain", "sd15_n1024")])
def test_recorded_coefficient_through_the_plug(gpu_device, route, shape):
    """One CrossAttention layer of each product route, called with a context that carries the recorder: the recorded map is the one of
    fp64 torch with qk.max() taken from the materialised scores -- i.e. the c[b] of the probabilities launch is the attention launch's."""
    import pww_hip
    from pww_hip import attention
    from pww_hip.conditioning import PwWContext
    dev, dtype, sigma = gpu_device, torch.float16, 7.84
    case = cases.make_attention_case(shape)
    mod = case["attn_cross"].to(dev, dtype)
    hidden = case["hidden"].to(dev, dtype)
    H, N = case["H"], case["N"]
    if route == "plain":       # a tensor-valued coefficient: the weight function leaves the symbolic form
        wf = lambda w, sigma, qk: 0.4 * w * math.log(1 + sigma) * qk.max().materialize()  # noqa: E731
    else:
        wf = cases.weight_fn_runner
    seen, used = [], []
    real = pww_hip.ops.attention

    def spy(*a, **kw):
        used.append((a[0], a[1]))
        seen.append(pww_hip.ops.attention_route(kw.get("bias") is not None, kw.get("stat"), kw.get("scratch"), kw.get("parts"), a[1].shape[1])
                    + ("+parts" if kw.get("parts") is not None else ""))
        return real(*a, **kw)

    try:
        with pww_hip.record_attention_maps() as rec:
            ctx = PwWContext({"CONTEXT_TENSOR": case["ctx"].to(dev, dtype), f"CROSS_ATTENTION_WEIGHT_{N}": case["w"].to(dev),
                              "SIGMA": torch.tensor(sigma), "WEIGHT_FUNCTION": wf, attention.ATTN_RECORDER: rec})
            pww_hip.ops.attention = spy
            try:
                pww_hip.inj_forward(mod, hidden, ctx)
            finally:
                pww_hip.ops.attention = real
        assert seen == [{"qproj": "parts+parts", "qk_parts": "parts+parts", "plain": "plain"}[route]], seen
        maps = rec.maps()
        assert maps.counts == {N: 1}
        got = maps.raw(N).reshape(1, N, 77)
        q, k = used[0]          # the rounded q / k the attention launch read (the qproj route forms Q in its own GEMM)
        D = q.shape[-1] // H
        s64 = q.double().reshape(1, N, H, D).permute(0, 2, 1, 3) @ k.double().reshape(1, 77, H, D).permute(0, 2, 3, 1)
        c = torch.tensor([0.4 * math.log(1 + sigma)], dtype=torch.float32, device=dev) * s64.max().float()
        _check("plug %s %s" % (route, shape), got, q, k, H, mod.scale, case["w"].to(dev), c)
    finally:
        uninstall_all()


def _request(mode, tools, device, record, per_layer=False, wf=None, case=None, steps=4, seed=3):
    import pww_hip
    import paint_with_words as pw
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    img, ctx, prompt = case if case is not None else (cases.load_example_rgb(), cases.RUNNER_CONTEXT, cases.RUNNER_PROMPT)
    kw = dict(color_context=dict(ctx), color_map_image=Image.fromarray(img), input_prompt=prompt, num_inference_steps=steps, guidance_scale=7.5,
              seed=seed, device=str(device), weight_function=wf or cases.weight_fn_runner, preloaded_utils=tools, return_latents=True)
    old = pww_mod.DEFAULT_MODE
    pww_mod.DEFAULT_MODE = mode
    try:
        if not record:
            return pw.paint_with_words(**kw).clone(), None
        with pww_hip.record_attention_maps(per_layer=per_layer) as rec:
            lat = pw.paint_with_words(**kw).clone()
        return lat, rec.maps()
    finally:
        pww_mod.DEFAULT_MODE = old


def test_loop_with_recorder(gpu_device):
    """Tiny UNet, 4 steps, eager / folded / graph: the recorder changes no latent bit; folded and graph maps are bit-identical; eager and
    folded maps agree at the relative bar tests/test_loop_gpu.py uses between a batched graph run and eager runs (1e-2); toggling the recorder
    between graph-mode requests works in both orders; counts = layers x evaluations."""
    from pww_hip import attention
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    n_cross = sum(1 for name, _ in tools[1].named_modules() if name.endswith("attn2"))
    steps = 4
    try:
        lat, maps = {}, {}
        for mode in ("eager", "folded"):
            lat[mode + "_off"], _ = _request(mode, tools, gpu_device, False, steps=steps)
            lat[mode], maps[mode] = _request(mode, tools, gpu_device, True, steps=steps)
            assert torch.equal(lat[mode], lat[mode + "_off"]), "recorder changed the latents in %s mode" % mode
        # graph mode, toggled in both orders: off, on, off, on
        g_off1, _ = _request("graph", tools, gpu_device, False, steps=steps)
        g_on1, maps["graph"] = _request("graph", tools, gpu_device, True, steps=steps)
        g_off2, _ = _request("graph", tools, gpu_device, False, steps=steps)
        g_on2, maps2 = _request("graph", tools, gpu_device, True, steps=steps)
        g_on3, maps3 = _request("graph", tools, gpu_device, True, steps=steps)       # a second recorder that only REPLAYS the captured graph
        sampler = tools[1]._pww_samplers[(id(tools[4]), "graph")]
        assert sampler._graphed.captures == 4                                         # one per toggle, none for the repeat
        assert torch.equal(g_on1, g_off1) and torch.equal(g_off2, g_off1) and torch.equal(g_on2, g_off1) and torch.equal(g_on3, g_off1)
        maps["graph again"] = maps3
        for m in maps.values():
            assert sum(m.counts.values()) == n_cross * steps, (m.counts, n_cross, steps)
        assert maps["graph"].counts == maps["folded"].counts == maps["eager"].counts == maps3.counts
        for N in maps["folded"].resolutions:
            assert torch.equal(maps["folded"].raw(N), maps["graph"].raw(N)), "folded and graph maps differ at N = %d" % N
            assert torch.equal(maps2.raw(N), maps["graph"].raw(N)) and torch.equal(maps3.raw(N), maps["graph"].raw(N))
            d = rel_l2(maps["eager"].raw(N), maps["folded"].raw(N))
            print("N = %d: eager vs folded maps rel-L2 %.3e" % (N, d))
            assert d <= 1e-2
            sums = maps["graph"].raw(N).sum(-1)
            assert (sums - 1).abs().max().item() <= 1e-5 * 4
        assert attention.ATTN_RECORDER not in tools[1]._pww_samplers[(id(tools[4]), "graph")]._static_folded
    finally:
        uninstall_all()


def test_maps_follow_the_painted_regions(gpu_device):
    """With the bias dominating (5 x w, stripes of strength >= 0.2 ... 1.6) every painted phrase's map is brighter inside its stripe than
    outside; per_layer=True gives one map per cross-attention layer whose count-weighted mean is the default map."""
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    img, ctx, prompt = cases.stripes_case(8, 512)
    ctx = {color: v.split(",")[0] + ",1.0" for color, v in ctx.items()}       # strength 1 regions
    wf = lambda w, sigma, qk: 5 * w * math.log(1 + sigma) * qk.max()          # noqa: E731
    try:
        _, maps = _request("folded", tools, gpu_device, True, wf=wf, case=(img, ctx, prompt))
        _, per = _request("folded", tools, gpu_device, True, per_layer=True, wf=wf, case=(img, ctx, prompt))
        H, W = max(maps.resolutions.values())
        for i, (color, v) in enumerate(ctx.items()):
            word = v.split(",")[0]
            m = maps.phrase(word)[0]
            inside = torch.zeros(H, W, dtype=torch.bool, device=m.device)
            inside[:, i * W // 8:(i + 1) * W // 8] = True
            mi, mo = m[inside].mean().item(), m[~inside].mean().item()
            print("%s: inside %.4f outside %.4f" % (word, mi, mo))
            assert mi > mo, (word, mi, mo)
        layers = per.layers
        n_cross = sum(1 for name, _ in tools[1].named_modules() if name.endswith("attn2"))
        assert len(layers) == n_cross
        mix = sum(m.tokens(size=(H, W)) * m.count for m in layers) / sum(m.count for m in layers)
        torch.testing.assert_close(mix, maps.tokens(), rtol=1e-5, atol=1e-7)
        assert isinstance(maps.to_pil("alpha")[0], Image.Image)
    finally:
        uninstall_all()
