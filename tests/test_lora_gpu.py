"""LoRA adapters on the GPU: the low-rank kernel of libpww_hip_lora.so against an fp64 evaluation of its formula (yardstick: the stock-torch
formula on the same device), and the adapters through the sampler's three modes against the merged-UNet oracle loop."""
import pytest
import torch

import lora_cases as L

pytestmark = pytest.mark.gpu

HALF_ULP = {torch.float16: 2.0 ** -12, torch.bfloat16: 2.0 ** -9}
TOKENS, IN_FEATURES = (1, 63, 64, 65, 77, 130), (32, 96, 320)


@pytest.mark.parametrize("N,n_seg", [(16, 1), (48, 3), (96, 2), (960, 3)])
@pytest.mark.parametrize("rank", [32, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_kernel_against_fp64_and_the_torch_formula(gpu_device, dtype, rank, N, n_seg):
    """err = max |y - exact| / max |exact| over the four rows; the kernel's must be within 1.5 x the stock-torch formula's + half an ulp."""
    from pww_hip import ops, lora
    rows = L.Rows(L.ROW_ADAPTERS, L.ROW_SCALES, gpu_device)
    for T in TOKENS:
        for K in IN_FEATURES:
            case = L.kernel_case(T, K, N, n_seg, rank, dtype, gpu_device)
            exact = L.kernel_exact(case, dtype)
            before = case["ybuf"].clone()
            # the yardstick, on a copy of the same strided buffers
            ybuf_t = before.clone()
            ops.lora_update_torch(ybuf_t[:, :T, 8:8 + N], case["x"], case["A"], case["B"], rows.row_adapter, rows.row_scale, n_seg)
            lora.reset_stats()
            assert ops.lora_takes(case["y"], case["x"], case["A"], case["B"], n_seg)
            ops.lora_update(case["y"], case["x"], (case["A"], case["B"]), rows, n_seg)
            assert lora.stats() == {"kernel": 1, "declined": 0}
            scale = exact.abs().max().item()
            err_k = (case["y"].double().cpu() - exact).abs().max().item() / scale
            err_t = (ybuf_t[:, :T, 8:8 + N].double().cpu() - exact).abs().max().item() / scale
            print("lora %s rank %3d N %4d/%d T %3d K %3d: kernel %.3e torch %.3e" % (str(dtype)[6:], rank, N, n_seg, T, K, err_k, err_t))
            assert err_k <= 1.5 * err_t + HALF_ULP[dtype], (T, K, err_k, err_t)
            # rows without an adapter / with scale 0 keep their bits; so does everything around the view
            for r in (0, 3):
                assert torch.equal(case["y"][r], before[r, :T, 8:8 + N])
            mask = torch.ones_like(before, dtype=torch.bool)
            mask[:, :T, 8:8 + N] = False
            assert torch.equal(case["ybuf"][mask], before[mask]) and bool((case["ybuf"][mask] == L.SENTINEL).all())
            assert bool((case["xbuf"][..., K:] == L.SENTINEL).all())
            # bitwise repeatable
            again = before.clone()
            ops.lora_update(again[:, :T, 8:8 + N], case["x"], (case["A"], case["B"]), rows, n_seg)
            assert torch.equal(again, case["ybuf"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_kernel_under_graph_capture_and_a_new_assignment_on_replay(gpu_device, dtype):
    from pww_hip import ops
    T, K, N, n_seg, rank = 77, 96, 96, 2, 32
    rows = L.Rows(L.ROW_ADAPTERS, L.ROW_SCALES, gpu_device)
    case = L.kernel_case(T, K, N, n_seg, rank, dtype, gpu_device)
    before = case["ybuf"].clone()
    eager = before.clone()
    ops.lora_update(eager[:, :T, 8:8 + N], case["x"], (case["A"], case["B"]), rows, n_seg)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.lora_update(case["y"], case["x"], (case["A"], case["B"]), rows, n_seg)
    case["ybuf"].copy_(before)
    g.replay()
    assert torch.equal(case["ybuf"], eager)
    # the launch reads the assignment when it runs: other rows and scales on the same graph
    rows.row_adapter.copy_(torch.tensor([1, -1, 0, 1], dtype=torch.int32))
    rows.row_scale.copy_(torch.tensor([2.0, 1.0, 0.25, 1.0]))
    eager2 = before.clone()
    ops.lora_update(eager2[:, :T, 8:8 + N], case["x"], (case["A"], case["B"]), rows, n_seg)
    case["ybuf"].copy_(before)
    g.replay()
    assert torch.equal(case["ybuf"], eager2) and not torch.equal(eager2, eager)
    assert torch.equal(eager2[1], before[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# the adapters through the sampler: tiny UNet, R.STEPS steps, against the merged-UNet oracle loop (tests/golden/lora_oracle.npz)
import importlib      # noqa: E402
import warnings       # noqa: E402

import numpy as np    # noqa: E402
from PIL import Image  # noqa: E402

import pww_cases as cases           # noqa: E402
import region_prompt_cases as R     # noqa: E402
from gpu_util import install_unfused, uninstall_all, rel_l2, unfused_inj_forward      # noqa: E402

CAP = L.CAP
SKY, GROUND = list(L.REGIONS2)


def _tools(dtype, device, adapters=("a", "b"), config="tiny", **kw):
    from pww_hip import lora
    tools = cases.build_tools(config, dtype=dtype, device=device, **({"qk_gain": R.QK_GAIN} if config == "tiny" else {}), **kw)
    for name in adapters:
        lora.load_lora(tools[1], L.kohya_dict(L.adapter_factors(tools[1], name)), name)
    return tools


def unfused_lora_forward(module, hidden_states, context=None, mask=None):
    """gpu_util.unfused_inj_forward with the row's adapter behind every projection, by the stock-torch formula (ops.lora_update_torch: held
    to merged weights in fp64 by tests/test_lora_host.py) -- the reference's op sequence in the storage type, no kernel of this package."""
    from pww_hip import ops
    from oracle import pww_oracle as O
    lo = module.__dict__.get("_pww_lora")
    if lo is None:
        return unfused_inj_forward(module, hidden_states, context, mask)
    st = lo.state
    upd = lambda y, x, names: ops.lora_update_torch(y, x, *lo.stack(names), st.row_adapter, st.row_scale, 1)      # noqa: E731
    is_dict = isinstance(context, dict)
    ctx = hidden_states if context is None else (context["CONTEXT_TENSOR"] if is_dict else context)
    wdt = module.to_q.weight.dtype
    h, c = hidden_states.to(wdt), ctx.to(wdt)
    q, k, v = upd(module.to_q(h), h, ("to_q",)), upd(module.to_k(c), c, ("to_k",)), upd(module.to_v(c), c, ("to_v",))
    q, k, v = (O.split_heads(t, module.heads) for t in (q, k, v))
    scores = torch.matmul(q, k.transpose(-1, -2))
    bias = 0.0
    if is_dict:
        bias = context["WEIGHT_FUNCTION"](context[f"CROSS_ATTENTION_WEIGHT_{scores.shape[-2]}"], context["SIGMA"], scores)
    probs = ((scores.float() + bias) * module.scale).softmax(dim=-1)
    out = O.merge_heads(torch.matmul(probs.to(v.dtype), v), module.heads)
    return upd(module.to_out[0](out), out, ("to_out.0",))


def _install_unfused_lora(unet):
    for m in unet.modules():
        if m.__class__.__name__ == "CrossAttention":
            m.__class__.__call__ = unfused_lora_forward


def _hip_loop(tools, device, mode, regions=None, steps=L.STEPS, seed=0, unfused=None, **kw):
    import paint_with_words as pw
    from pww_hip import sampler as S
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    old, pww_mod.DEFAULT_MODE = pww_mod.DEFAULT_MODE, mode
    orig_install = S.install
    if unfused is not None:
        S.install = unfused        # calibration path: same driver, attention as unfused torch ops
    try:
        return pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()),
                                   input_prompt=cases.RUNNER_PROMPT, num_inference_steps=steps, guidance_scale=R.GUIDANCE, seed=seed, device=str(device),
                                   weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True,
                                   region_prompts=None if regions is None else dict(regions), **kw).clone()
    finally:
        S.install = orig_install
        pww_mod.DEFAULT_MODE = old
        if unfused is not None:
            uninstall_all()


@pytest.fixture(scope="module")
def oracle_latents():
    return L.recorded()


def _no_lora_warnings(caught):
    assert not [str(w.message) for w in caught if "lora" in str(w.message).lower()]


@pytest.mark.parametrize("mode", ["eager", "folded", "graph"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_tiny_loop_with_a_global_adapter_vs_the_merged_oracle(gpu_device, oracle_latents, dtype, mode):
    """lora="a" alone behaves like merged weights. Yardstick: the unfused torch ops on a UNet of the same dtype with the adapter merged."""
    from pww_hip import lora
    tools = _tools(dtype, gpu_device)
    try:
        lora.reset_stats()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            lat = _hip_loop(tools, gpu_device, mode, lora=L.GLOBAL)
        stats = lora.stats()
        plain = _hip_loop(tools, gpu_device, mode)
        plain_tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=R.QK_GAIN)
        merged = L.merged(plain_tools[1], L.adapter_factors(plain_tools[1], L.GLOBAL[0]), L.GLOBAL[1])
        base = _hip_loop((plain_tools[0], merged) + tuple(plain_tools[2:]), gpu_device, "eager", unfused=install_unfused)
    finally:
        uninstall_all()
    d, d0, d_plain, visible = rel_l2(lat, oracle_latents["global"]), rel_l2(base, oracle_latents["global"]), rel_l2(plain, oracle_latents["without"]), rel_l2(lat, plain)
    print(f"lora global tiny {dtype} {mode}: rel-L2 hip {d:.3e} unfused-torch {d0:.3e}; without {d_plain:.3e}; with vs without {visible:.3e}; {stats}")
    assert d <= 1.5 * d0 + 2e-3
    assert d <= CAP[dtype]
    assert d_plain <= CAP[dtype]
    assert visible >= 2 * CAP[dtype]
    assert stats["declined"] == 0 and stats["kernel"] > 0
    _no_lora_warnings(caught)


@pytest.mark.parametrize("mode", ["eager", "folded", "graph"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_tiny_loop_with_an_adapter_per_region_vs_the_merged_oracle(gpu_device, oracle_latents, dtype, mode):
    """Two regions, adapter "a" on one and "b" on the other, none on the base and unconditional rows; then the two swapped."""
    from pww_hip import lora
    tools = _tools(dtype, gpu_device)
    try:
        lora.reset_stats()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            lat = _hip_loop(tools, gpu_device, mode, L.REGIONS2, region_loras=dict(L.REGION_LORAS))
            swapped = _hip_loop(tools, gpu_device, mode, L.REGIONS2, region_loras=dict(L.SWAPPED_LORAS))
        stats = lora.stats()
        plain = _hip_loop(tools, gpu_device, mode, L.REGIONS2)
        base = _hip_loop(_tools(dtype, gpu_device), gpu_device, "eager", L.REGIONS2, region_loras=dict(L.REGION_LORAS), unfused=_install_unfused_lora)
    finally:
        uninstall_all()
    d, d0 = rel_l2(lat, oracle_latents["regions"]), rel_l2(base, oracle_latents["regions"])
    d_plain, visible = rel_l2(plain, oracle_latents["regions_without"]), rel_l2(lat, plain)
    d_s, moved = rel_l2(swapped, oracle_latents["swapped"]), rel_l2(swapped, lat)
    print(f"lora regions tiny {dtype} {mode}: rel-L2 hip {d:.3e} unfused-torch {d0:.3e}; without {d_plain:.3e}; with vs without {visible:.3e}; "
          f"swapped vs its oracle {d_s:.3e}, vs unswapped {moved:.3e}; {stats}")
    assert d <= 1.5 * d0 + 2e-3
    assert d <= CAP[dtype] and d_s <= CAP[dtype] and d_plain <= CAP[dtype]
    assert visible >= 2 * CAP[dtype] and moved >= 2 * CAP[dtype]
    assert stats["declined"] == 0 and stats["kernel"] > 0
    _no_lora_warnings(caught)


def test_graph_replays_a_new_assignment_and_captures_again_on_load(gpu_device):
    from pww_hip import lora
    tools = _tools(torch.float16, gpu_device)
    steps = 4
    other = dict(lora=("b", 0.5), region_loras={SKY: ("b", 0.75), GROUND: ("a", -0.5)})
    try:
        a = _hip_loop(tools, gpu_device, "graph", L.REGIONS2, steps=steps, seed=1, lora=L.GLOBAL, region_loras=dict(L.REGION_LORAS))
        sampler = tools[1]._pww_samplers[(id(tools[4]), "graph")]
        assert sampler._graphed.captures == 1 and len(sampler._graphed.graphs) == 1
        b = _hip_loop(tools, gpu_device, "graph", L.REGIONS2, steps=steps, seed=1, **other)
        assert sampler._graphed.captures == 1                               # another assignment, other scales: replayed
        b_eager = _hip_loop(tools, gpu_device, "eager", L.REGIONS2, steps=steps, seed=1, **other)
        print("graph replay with a new assignment vs eager %.3e; vs the first assignment %.3e" % (rel_l2(b, b_eager), rel_l2(a, b)))
        assert rel_l2(b, b_eager) <= 2e-2 and rel_l2(a, b) > 4e-2           # a stale row, scale or K|V projection would show as O(1)
        none = _hip_loop(tools, gpu_device, "graph", L.REGIONS2, steps=steps, seed=1)
        assert sampler._graphed.captures == 1                               # adapters loaded, no row uses one: the same graph
        lora.load_lora(tools[1], L.kohya_dict(L.make_factors(tools[1], seed=13, rank=4, gain=3.0)), "c")
        c = _hip_loop(tools, gpu_device, "graph", L.REGIONS2, steps=steps, seed=1, **other)
        assert sampler._graphed.captures == 2 and rel_l2(c, b) <= 2e-2      # a third adapter: captured again, once
        c2 = _hip_loop(tools, gpu_device, "graph", L.REGIONS2, steps=steps, seed=1, lora="c")
        assert sampler._graphed.captures == 2 and rel_l2(c2, c) > 4e-2
        for name in ("a", "b", "c"):
            lora.unload_lora(tools[1], name)
        off = _hip_loop(tools, gpu_device, "graph", L.REGIONS2, steps=steps, seed=1)
        assert sampler._graphed.captures == 3
        never = _hip_loop(_tools(torch.float16, gpu_device, adapters=()), gpu_device, "graph", L.REGIONS2, steps=steps, seed=1)
        assert torch.equal(off, never)                                      # nothing of the adapters is left
        assert rel_l2(none, never) <= 2e-2                                  # (rows of -1 are the adapter-free computation, on other launches)
    finally:
        uninstall_all()


def test_batch_with_per_image_region_loras_equals_the_single_calls(gpu_device):
    import paint_with_words as pw
    tools = _tools(torch.float16, gpu_device)
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    old, pww_mod.DEFAULT_MODE = pww_mod.DEFAULT_MODE, "folded"
    steps, per = 4, [dict(L.REGION_LORAS), dict(L.SWAPPED_LORAS), None]
    try:
        kw = dict(num_inference_steps=steps, guidance_scale=R.GUIDANCE, device=str(gpu_device), weight_function=cases.weight_fn_runner, preloaded_utils=tools,
                  return_latents=True, region_prompts=dict(L.REGIONS2), lora=("a", 0.5))
        image = Image.fromarray(cases.load_example_rgb())
        batched = pw.paint_with_words_batch(dict(cases.RUNNER_CONTEXT), image, cases.RUNNER_PROMPT, [3, 3, 3], region_loras=per, **kw).clone()
        single = torch.cat([pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=image, input_prompt=cases.RUNNER_PROMPT, seed=3,
                                                region_loras=p, **kw).clone() for p in per])
    finally:
        pww_mod.DEFAULT_MODE = old
        uninstall_all()
    d = [rel_l2(batched[i:i + 1], single[i:i + 1]) for i in range(3)]
    apart = [rel_l2(single[i:i + 1], single[j:j + 1]) for i, j in ((0, 1), (0, 2), (1, 2))]
    print("per-image region_loras, 3-image batch vs single calls: %s; the three requests apart by %s" % (["%.3e" % v for v in d], ["%.3e" % v for v in apart]))
    assert max(d) <= 2e-2 and min(apart) > 4e-2


def test_inpaint_pipeline_classes_and_the_recorder_with_adapters(gpu_device):
    import paint_with_words as pw
    import pww_hip
    from pww_hip import lora
    colors = list(cases.INPAINT_CONTEXT)
    regions = {colors[0]: "green aurora over a dark sky", colors[3]: "a frozen lake, cracked ice"}
    try:
        tools = cases.build_tools("tiny_inpaint", dtype=torch.float16, device=gpu_device)
        for name in ("a", "b"):
            lora.load_lora(tools[1], L.kohya_dict(L.adapter_factors(tools[1], name)), name)
        kw = dict(color_map_image=Image.fromarray(cases.load_aurora_rgb()), mask_image=cases.load_moon_mask(), init_image=Image.fromarray(cases.synthetic_init_image()),
                  input_prompt=cases.AURORA_PROMPT, num_inference_steps=4, guidance_scale=7.5, seed=81, device=str(gpu_device),
                  weight_function=cases.weight_fn_inpaint, preloaded_utils=tools, strength=1.0, return_latents=True, region_prompts=dict(regions))
        loras = dict(lora=("a", 0.5), region_loras={colors[3]: "b"})
        with_l = pw.paint_with_words_inpaint(color_context=dict(cases.INPAINT_CONTEXT), **loras, **kw).clone()
        without = pw.paint_with_words_inpaint(color_context=dict(cases.INPAINT_CONTEXT), **kw).clone()
        assert torch.isfinite(with_l).all() and rel_l2(with_l, without) > 4e-2
        both = pw.paint_with_words_inpaint_batch(dict(cases.INPAINT_CONTEXT), kw["color_map_image"], kw["mask_image"], kw["init_image"], cases.AURORA_PROMPT, [81, 81],
                                                 lora=loras["lora"], region_loras=[loras["region_loras"], None],
                                                 **{k: v for k, v in kw.items() if k not in ("color_map_image", "mask_image", "init_image", "input_prompt", "seed")})
        assert rel_l2(both[:1], with_l) <= 2e-2 and rel_l2(both[1:], with_l) > 1e-2
        vae, unet, text, tok, sch = tools
        pipe = pw.PaintWithWord_StableDiffusionInpaintPipeline(vae, text, tok, unet, sch)
        call = dict(prompt=cases.AURORA_PROMPT, image=kw["init_image"], mask_image=kw["mask_image"], color_map_image=kw["color_map_image"],
                    color_context=dict(cases.INPAINT_CONTEXT), weight_function=cases.weight_fn_inpaint, num_inference_steps=3, guidance_scale=7.5,
                    height=512, width=512, seed=81, output_type="np")
        plain = pipe(**call).images[0]
        pipe.region_prompts, pipe.lora, pipe.region_loras = dict(regions), "a", {colors[0]: ("b", 0.5)}
        painted = pipe(**call).images[0]
        assert plain.shape == painted.shape == (512, 512, 3) and np.isfinite(painted).all() and np.abs(painted - plain).mean() > 1e-3
        uninstall_all()
        vae, unet, text, tok, sch = tools = _tools(torch.float16, gpu_device)
        pipe = pw.PaintWithWord_StableDiffusionPipeline(vae, text, tok, unet, sch)
        call = dict(prompt=cases.RUNNER_PROMPT, color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()),
                    num_inference_steps=3, guidance_scale=7.5, weight_function=cases.weight_fn_runner, output_type="np")
        plain = pipe(**call).images[0]
        pipe.lora = ("b", 1.0)
        painted = pipe(**call).images[0]
        assert np.isfinite(painted).all() and np.abs(painted - plain).mean() > 1e-3
        pipe.lora = "missing"
        with pytest.raises(ValueError, match="not loaded"):
            pipe(**call)
        # the attention-map recorder under a LoRA request: other maps than the adapter-free ones, and no latent bit changes
        maps = {}
        for name, more in (("lora", dict(lora=L.GLOBAL)), ("plain", {})):
            lat = _hip_loop(tools, gpu_device, "folded", steps=3, **more)
            with pww_hip.record_attention_maps() as rec:
                lat_rec = _hip_loop(tools, gpu_device, "folded", steps=3, **more)
            assert torch.equal(lat, lat_rec), name
            maps[name] = rec.maps()
        assert maps["lora"].counts == maps["plain"].counts and sum(maps["lora"].counts.values()) > 0
        for N in maps["lora"].resolutions:
            d = rel_l2(maps["lora"].raw(N), maps["plain"].raw(N))
            print("N = %d: maps with the adapter vs without, rel-L2 %.3e" % (N, d))
            assert d > 1e-2
    finally:
        uninstall_all()
