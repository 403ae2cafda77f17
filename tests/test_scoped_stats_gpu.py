"""Per-head / per-row score statistics on the GPU: the launches of libpww_hip_scope.so call by call (through pww_hip.ops), through
inj_forward against the reference's goldens, and through whole hipGraph-mode requests.

Bars (none of them new):
  * per call against fp64 torch on the same rounded inputs: max|d| <= 2e-3 max|O| fp16 / 1.6e-2 max|O| bf16 (gpu_util.TOL);
  * the folded head statistics against fp64 torch: 1e-6 relative to the largest score (the header's statement for partials; sums per element,
    as tests/test_long_prompt_gpu.py normalises them);
  * the two routes of one weight function (libpww_hip_scope.so / materialised scores) among each other: 2 x TOL max|O|;
  * inj_forward against the reference's goldens: 1.5 x the unfused torch path on the same GPU + 2e-3 max|O| (tests/test_attention_gpu.py);
  * final latents of the tiny loop, fp16: rel-L2 <= 2e-2 against the fp32 CPU oracle loop and <= 1.5 x the unfused torch path + 2e-3
    (tests/test_loop_gpu.py).
"""
import copy
import ctypes
import math
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import pww_cases as cases
from gpu_util import TOL, unfused_inj_forward, uninstall_all, rel_l2
from oracle import pww_oracle as O

pytestmark = pytest.mark.gpu


def wf_head(w, s, qk):
    return 0.4 * w * math.log(1 + s) * qk.amax(dim=(1, 2), keepdim=True)


def wf_row(w, s, qk):
    return 0.5 * w * math.log(1 + s ** 2) * qk.std(dim=-1, keepdim=True)


@pytest.fixture(scope="module")
def scope_lib(gpu_device):
    """libpww_hip_scope.so, built in-tree when missing (no conftest of its own: the module builds / locates the library itself)."""
    import build as pww_build
    path = pww_build.build_scope()
    assert os.path.isfile(path)
    from pww_hip import _lib
    lib = _lib.load_scope()
    assert lib is not None
    return lib


def _heads(t, H):
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H).permute(0, 2, 1, 3)


def _stat64(s, kind, scope):
    """The statistic of the fp64 scores s [B, H, N, M]: scope "head" -> [B, H, 1, 1], "row" -> [B, H, N, 1], "image" -> [B, 1, 1, 1]."""
    from pww_hip import ops
    dims = {"head": (2, 3), "row": (3,), "image": (1, 2, 3)}[scope]
    if kind == ops.STAT_MAX:
        return s.amax(dims, keepdim=True)
    if kind == ops.STAT_MIN:
        return s.amin(dims, keepdim=True)
    if kind == ops.STAT_MEAN:
        return s.mean(dims, keepdim=True)
    if kind == ops.STAT_STD:
        return s.std(dims, keepdim=True)
    return s.abs().amax(dims, keepdim=True)


def _oracle(q, k, v, H, scale, w, kind, scope, scalar, gate=None):
    """softmax((Q K^T + c w) scale) V in fp64 on the rounded q / k / v, c = scalar * stat * gate[b]."""
    B = q.shape[0]
    qh, kh, vh = _heads(q.double(), H), _heads(k.double().expand(B, -1, -1), H), _heads(v.double().expand(B, -1, -1), H)
    s = qh @ kh.transpose(-1, -2)
    c = scalar * _stat64(s, kind, scope) if kind is not None else torch.full((B, 1, 1, 1), float(scalar), dtype=torch.float64, device=q.device)
    if gate is not None:
        c = c * gate.double().reshape(B, 1, 1, 1)
    wb = w.double() if w.dim() == 4 else w.double().reshape(1, 1, *w.shape)
    o = ((s + c * wb) * scale).softmax(-1) @ vh
    return o.permute(0, 2, 1, 3).reshape(B, q.shape[1], -1), s


def _scoped(q, k, v, H, scale, w, kind, scope, scalar, gate=None, coeff_dev=None, stats_out=None, parts=None):
    from pww_hip import ops
    sc = ops.SCOPE_HEAD if scope == "head" else ops.SCOPE_ROW
    if scope == "head" and parts is None:
        parts = ops.scope_head_parts(q, k, H, kind, gate=gate)
    return ops.attention_scoped(q, k, v, H, scale, w, kind, sc, scalar, gate=gate, parts=parts, stats_out=stats_out, coeff_dev=coeff_dev)


def _map(N, M, g, dev):
    """a dense [N, M] weight map: a few region columns (none past M), random row sets, strengths 0.2 .. 1.5"""
    w = torch.zeros(N, M)
    for c in sorted({0, min(3, M - 1), min(17, M - 1), M - 1}):
        rows = torch.rand(N, generator=g) < 0.4
        w[rows, c] = 0.2 + 1.3 * float(torch.rand((), generator=g))
    return w.to(dev)


SHAPES = [(2, 3, 70, 77, 40), (1, 2, 33, 128, 64), (1, 1, 32, 5, 8), (2, 8, 256, 77, 160), (1, 2, 1056, 77, 40)]
KINDS = ["MAX", "MIN", "MEAN", "STD", "ABSMAX"]
_inputs = {}


def _case(shape, dtype, dev):
    """Seeded q / k / v / map of one shape and the fp64 scores, made once and shared by every test that needs them."""
    key = (shape, dtype)
    if key not in _inputs:
        B, H, N, M, D = shape
        g = torch.Generator().manual_seed(1234 + sum(shape))
        q = torch.randn(B, N, H * D, generator=g).to(dev, dtype)
        k = torch.randn(1, M, H * D, generator=g).to(dev, dtype)
        v = torch.randn(1, M, H * D, generator=g).to(dev, dtype)
        _inputs[key] = (q, k, v, _map(N, M, g, dev))
    return _inputs[key]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind_name", KINDS)
@pytest.mark.parametrize("scope", ["head", "row"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_parity_through_ops(scope_lib, gpu_device, shape, scope, kind_name, dtype):
    from pww_hip import ops
    B, H, N, M, D = shape
    kind = getattr(ops, "STAT_" + kind_name)
    q, k, v, w = _case(shape, dtype, gpu_device)
    scale, scalar = D ** -0.5, (0.9 if kind in (ops.STAT_STD, ops.STAT_MEAN) else 0.4 * math.log(1 + 7.84) * (0.35 if scope == "row" else 0.25))
    stats_out = torch.zeros(B, H, 4, dtype=torch.float64, device=gpu_device) if scope == "head" else None
    out = _scoped(q, k, v, H, scale, w, kind, scope, scalar, stats_out=stats_out)
    again = _scoped(q, k, v, H, scale, w, kind, scope, scalar)
    assert torch.equal(out, again), "two identical launches differ"
    ref, s = _oracle(q, k, v, H, scale, w, kind, scope, scalar)
    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    print("%s %s %s %s: max err / max|O| = %.3e (bar %.1e)" % (shape, scope, kind_name, str(dtype)[6:], err, TOL[dtype]))
    assert not torch.isnan(out).any()
    assert err <= TOL[dtype], err
    if scope == "head":
        big, count = s.abs().max().item(), float(N * M)
        want = torch.stack([s.amax((2, 3)), s.amin((2, 3)), s.sum((2, 3)), (s * s).sum((2, 3))], dim=-1)
        fields = {ops.STAT_MAX: [0], ops.STAT_MIN: [1], ops.STAT_ABSMAX: [0, 1], ops.STAT_MEAN: [2], ops.STAT_STD: [2, 3]}[kind]
        norm = [big, big, big * count, big * big * count]
        serr = max((stats_out[..., f] - want[..., f]).abs().max().item() / norm[f] for f in fields)
        print("    folded statistics: %.3e of the largest score (bar 1e-6), %d partial(s) per head" % (serr, (N + 127) // 128))
        assert serr <= 1e-6, serr


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_scope_is_really_applied(scope_lib, gpu_device, dtype):
    """Head h's keys scaled by (h + 1), the queries by a ramp over the rows: per-head, per-row and per-image maxima are far apart. First the
    three ORACLE outputs must differ pairwise by at least 20 TOL max|O|; then each GPU output must match its own oracle."""
    from pww_hip import ops
    dev = gpu_device
    B, H, N, M, D = 1, 4, 96, 77, 40
    g = torch.Generator().manual_seed(77)
    ramp = torch.linspace(0.25, 1.75, N).reshape(1, N, 1)
    q = (torch.randn(B, N, H * D, generator=g) * ramp).to(dev, dtype)
    k = (torch.randn(1, M, H, D, generator=g) * torch.arange(1, H + 1).reshape(1, 1, H, 1) * 0.5).reshape(1, M, H * D).to(dev, dtype)
    v = torch.randn(1, M, H * D, generator=g).to(dev, dtype)
    w = _map(N, M, g, dev)
    scale, scalar, kind = D ** -0.5, 0.5, ops.STAT_MAX
    refs = {sc: _oracle(q, k, v, H, scale, w, kind, sc, scalar)[0] for sc in ("head", "row", "image")}
    top = max(r.abs().max().item() for r in refs.values())
    for a, b in (("head", "row"), ("head", "image"), ("row", "image")):
        gap = (refs[a] - refs[b]).abs().max().item()
        print("oracle %s vs %s: %.3e of max|O| (needs >= %.3e)" % (a, b, gap / top, 20 * TOL[dtype]))
        assert gap >= 20 * TOL[dtype] * top, (a, b, gap, top)
    outs = {"head": _scoped(q, k, v, H, scale, w, kind, "head", scalar), "row": _scoped(q, k, v, H, scale, w, kind, "row", scalar),
            "image": ops.attention(q, k, v, H, scale, bias=w, stat=(None, kind, scalar), parts=ops.qk_parts(q, k, H, kind))}
    for sc, out in outs.items():
        err = (out.double() - refs[sc]).abs().max().item() / refs[sc].abs().max().item()
        print("%s scope on the GPU: %.3e (bar %.1e)" % (sc, err, TOL[dtype]))
        assert err <= TOL[dtype], (sc, err)


@pytest.mark.parametrize("scope", ["head", "row"])
def test_gate_is_a_factor_and_zero_means_no_bias(scope_lib, gpu_device, scope):
    from pww_hip import ops
    dev, dtype = gpu_device, torch.float16
    B, H, N, M, D = 4, 2, 160, 77, 40
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, N, H * D, generator=g).to(dev, dtype)
    k, v = torch.randn(1, M, H * D, generator=g).to(dev, dtype), torch.randn(1, M, H * D, generator=g).to(dev, dtype)
    w = _map(N, M, g, dev)
    gate = torch.tensor([1.0, 0.0, 0.5, -1.0], device=dev)
    scale, scalar, kind = D ** -0.5, 1.2, ops.STAT_STD
    parts = None
    if scope == "head":
        nparts = (N + 127) // 128
        parts = torch.full((B, H, nparts, 4), -12345.0, dtype=torch.float64, device=dev)
        fresh = ops.scope_head_parts(q, k, H, kind, gate=gate)
        assert fresh.shape == parts.shape
        # the launch itself into the pre-filled buffer: image 1's rows keep the sentinel
        from pww_hip import _lib
        d = ops._desc(q, k, None, None, H, 1.0)
        _lib.check(scope_lib.pww_scope_head_parts(ops._ptr(q), ops._ptr(k), ops._ptr(gate), ctypes.byref(d), int(kind), ops._ptr(parts),
                                                  parts.numel() * 8, ops._stream()), "pww_scope_head_parts", scope_lib)
        assert bool((parts[1] == -12345.0).all()) and not bool((parts[[0, 2, 3]] == -12345.0).any())
        assert torch.equal(parts[[0, 2, 3]], fresh[[0, 2, 3]])
    out = _scoped(q, k, v, H, scale, w, kind, scope, scalar, gate=gate, parts=parts)
    ref, _ = _oracle(q, k, v, H, scale, w, kind, scope, scalar, gate=gate)
    top = ref.abs().max().item()
    plain = ops.attention(q[1:2], k, v, H, scale)
    assert (out[1:2].double() - plain.double()).abs().max().item() <= TOL[dtype] * plain.double().abs().max().item()
    for b in range(B):
        err = (out[b].double() - ref[b]).abs().max().item() / top
        print("%s scope, image %d (gate %g): %.3e" % (scope, b, gate[b].item(), err))
        assert err <= TOL[dtype], (b, err)
    # the factor is really multiplied in: gate 0.5 and -1 give something else than gate 1
    one, _ = _oracle(q, k, v, H, scale, w, kind, scope, scalar)
    assert (one[2] - ref[2]).abs().max().item() > 20 * TOL[dtype] * top and (one[3] - ref[3]).abs().max().item() > 20 * TOL[dtype] * top


@pytest.mark.parametrize("scope", ["head", "row"])
def test_device_word_replaces_the_scalar(scope_lib, gpu_device, scope):
    from pww_hip import ops
    dev, dtype = gpu_device, torch.bfloat16
    q, k, v, w = _case(SHAPES[0], dtype, dev)
    B, H, N, M, D = SHAPES[0]
    scale, kind = D ** -0.5, ops.STAT_MAX
    word = torch.tensor([0.25], dtype=torch.float32, device=dev)
    by_value = _scoped(q, k, v, H, scale, w, kind, scope, 0.25)
    by_word = _scoped(q, k, v, H, scale, w, kind, scope, 123.0, coeff_dev=word)      # (the by-value argument is ignored)
    assert torch.equal(by_value, by_word)
    word.fill_(0.0625)
    after = _scoped(q, k, v, H, scale, w, kind, scope, 123.0, coeff_dev=word)
    assert torch.equal(after, _scoped(q, k, v, H, scale, w, kind, scope, 0.0625)) and not torch.equal(after, by_value)


def _ctx(case, wf, dev, dtype, sigma=7.8399, **extra):
    N = case["N"]
    d = {"CONTEXT_TENSOR": case["ctx"].to(dev, dtype), "CROSS_ATTENTION_WEIGHT_%d" % N: case["w"].to(dev), "SIGMA": torch.tensor(sigma), "WEIGHT_FUNCTION": wf}
    d.update(extra)
    return d


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", ["sd15_n64", "sd15_n256", "sd21_n576"])
def test_inj_forward_takes_the_new_route(scope_lib, gpu_device, shape, dtype, monkeypatch):
    """wf_head / wf_row through the plug: NO "materialising" warning (on the parent commit the scores are materialised: this fails there),
    agreement with the reference's goldens, with the CPU oracle on the rounded module, and with the materialised route (PWW_SCOPED_STATS=0),
    which does warn."""
    import pww_hip
    from pww_hip import attention as A
    dev = gpu_device
    g = np.load(os.path.join(cases.GOLDEN, "attn_scoped_%s.npz" % shape))
    case = cases.make_attention_case(shape)
    rows = torch.from_numpy(g["rows"])
    mod_ref = copy.deepcopy(case["attn_cross"]).to(dtype).float()      # (the CPU oracle's module: the same weights, rounded to the storage type)
    mod = case["attn_cross"].to(dev, dtype)
    hidden = case["hidden"].to(dev, dtype)
    for key, wf in (("head", wf_head), ("row", wf_row)):
        A._warned.discard("materialize")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            y = pww_hip.inj_forward(mod, hidden, _ctx(case, wf, dev, dtype))
        assert not [c for c in caught if "materialising" in str(c.message)], "the scores were materialised"
        assert "materialize" not in A._warned
        # the CPU oracle on the same rounded weights and inputs
        ctx_ref = {"CONTEXT_TENSOR": case["ctx"].to(dtype).float(), "CROSS_ATTENTION_WEIGHT_%d" % case["N"]: case["w"], "SIGMA": torch.tensor(7.8399),
                   "WEIGHT_FUNCTION": wf}
        ref = O.inj_forward(mod_ref, case["hidden"].to(dtype).float(), ctx_ref)
        err = (y.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
        # the reference's golden (fp32, un-rounded weights): calibrated by the unfused torch path on this GPU
        gold = torch.from_numpy(g[key])
        y_unf = unfused_inj_forward(mod, hidden, _ctx(case, wf, dev, dtype))[0, rows].float().cpu()
        e_g, e_unf, top = (y[0, rows].float().cpu() - gold).abs().max().item(), (y_unf - gold).abs().max().item(), gold.abs().max().item()
        # the materialised route of the same call
        monkeypatch.setattr(A, "SCOPED_STATS", False)
        A._warned.discard("materialize")
        with pytest.warns(UserWarning, match="materialising"):
            y_old = pww_hip.inj_forward(mod, hidden, _ctx(case, wf, dev, dtype))
        monkeypatch.setattr(A, "SCOPED_STATS", True)
        e_route = (y.float() - y_old.float()).abs().max().item() / y_old.float().abs().max().item()
        print("%s %s %s: vs oracle %.3e (bar %.1e), vs golden %.3e (unfused torch %.3e), vs materialised route %.3e (bar %.1e)"
              % (shape, key, str(dtype)[6:], err, TOL[dtype], e_g / top, e_unf / top, e_route, 2 * TOL[dtype]))
        assert err <= TOL[dtype], (key, err)
        assert e_g <= 1.5 * e_unf + 2e-3 * top and e_g <= (2e-2 if dtype == torch.float16 else 8e-2) * top, (key, e_g, e_unf, top)
        assert e_route <= 2 * TOL[dtype], (key, e_route)


def test_batched_statistics_are_per_image(scope_lib, gpu_device):
    """Batch 3 with a shared prompt: the statistics are per (image, head) / per row -- each image equals its own batch-1 call."""
    import pww_hip
    case = cases.make_attention_case("sd15_n256", seed=4)
    dev, dtype = gpu_device, torch.float16
    mod = case["attn_cross"].to(dev, dtype)
    g = torch.Generator().manual_seed(9)
    hidden = torch.randn(3, 256, 1280, generator=g).to(dev, dtype) * torch.tensor([1.0, 2.0, 0.5], device=dev, dtype=dtype)[:, None, None]
    for wf in (wf_head, wf_row):
        batched = pww_hip.inj_forward(mod, hidden, _ctx(case, wf, dev, dtype, sigma=5.0))
        for i in range(3):
            single = pww_hip.inj_forward(mod, hidden[i:i + 1], _ctx(case, wf, dev, dtype, sigma=5.0))
            assert (batched[i:i + 1].float() - single.float()).abs().max() <= TOL[dtype] * single.float().abs().max()
        assert (batched[0].float() - batched[1].float()).abs().max() > 0.05 * batched[0].float().abs().max()


def test_folded_cfg_rows_are_gated(scope_lib, gpu_device):
    """A CFG-folded context (ROW_GATE / GATED_ROWS): the conditional rows equal the batch-1 call, the unconditional rows the bias-free one."""
    import pww_hip
    from pww_hip.attention import ROW_GATE, GATED_ROWS
    case = cases.make_attention_case("sd15_n256", seed=6)
    dev, dtype = gpu_device, torch.float16
    mod = case["attn_cross"].to(dev, dtype)
    g = torch.Generator().manual_seed(3)
    hidden = (torch.randn(2, 256, 1280, generator=g) * torch.tensor([1.0, 1.7])[:, None, None]).to(dev, dtype)
    ctx_c, ctx_u = torch.randn(1, 77, 768, generator=g).to(dev, dtype), torch.randn(1, 77, 768, generator=g).to(dev, dtype)
    w, sig = case["w"].to(dev), torch.tensor(6.0)
    for wf in (wf_head, wf_row):
        folded = {"CONTEXT_TENSOR": torch.cat([ctx_c.expand(2, -1, -1), ctx_u.expand(2, -1, -1)]).contiguous(), "CROSS_ATTENTION_WEIGHT_256": w,
                  "SIGMA": sig, "WEIGHT_FUNCTION": wf, ROW_GATE: torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev), GATED_ROWS: 2}
        y = pww_hip.inj_forward(mod, torch.cat([hidden, hidden]), folded).float()
        for i in range(2):
            yc = pww_hip.inj_forward(mod, hidden[i:i + 1], {"CONTEXT_TENSOR": ctx_c, "CROSS_ATTENTION_WEIGHT_256": w, "SIGMA": sig, "WEIGHT_FUNCTION": wf}).float()
            yu = pww_hip.inj_forward(mod, hidden[i:i + 1], {"CONTEXT_TENSOR": ctx_u, "CROSS_ATTENTION_WEIGHT_256": 0, "SIGMA": sig,
                                                            "WEIGHT_FUNCTION": lambda w, sigma, qk: 0.0}).float()
            tol = TOL[dtype] * yc.abs().max().item()
            assert (y[i:i + 1] - yc).abs().max().item() <= tol
            assert (y[2 + i:3 + i] - yu).abs().max().item() <= tol
            assert (yc - yu).abs().max().item() > 20 * tol      # the bias is far from a no-op here


def _graph_request(wf, dev, steps=4, fused=True):
    """One hipGraph-mode request on fresh tiny tools -> (final latents, the sampler's capture count)."""
    import importlib
    import paint_with_words as pw
    from pww_hip import sampler as S
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    tools = cases.build_tools("tiny", dtype=torch.float16, device=dev)
    old, orig_install = pww_mod.DEFAULT_MODE, S.install
    pww_mod.DEFAULT_MODE = "graph" if fused else "eager"
    try:
        if not fused:
            from gpu_util import install_unfused
            S.install = install_unfused
        lat = pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()),
                                  input_prompt=cases.RUNNER_PROMPT, num_inference_steps=steps, guidance_scale=7.5, seed=0, device=str(dev),
                                  weight_function=wf, preloaded_utils=tools, return_latents=True)
        captures = tools[1]._pww_samplers[(id(tools[4]), "graph")]._graphed.captures if fused else None
        return lat.float().cpu(), captures
    finally:
        pww_mod.DEFAULT_MODE, S.install = old, orig_install
        uninstall_all()


def _oracle_loop(wf, steps=4):
    tools_cpu = cases.build_tools("tiny")
    O.install_oracle_attention(tools_cpu[1])
    try:
        return O.paint_with_words_latents(dict(cases.RUNNER_CONTEXT), cases.load_example_rgb(), cases.RUNNER_PROMPT, tools_cpu[1], tools_cpu[2],
                                          tools_cpu[3], tools_cpu[4], num_inference_steps=steps, guidance_scale=7.5, seed=0, weight_function=wf)
    finally:
        uninstall_all()


def _wf_switch(w, s, qk):
    return wf_head(w, s, qk) if float(s) > 3.0 else wf_row(w, s, qk)


@pytest.mark.parametrize("name,wf,want_captures", [("head", wf_head, 1), ("row", wf_row, 1), ("switch", _wf_switch, 2)])
def test_graph_mode_serves_every_step_with_one_capture(scope_lib, gpu_device, name, wf, want_captures):
    """A 4-step graph-mode request: ONE captured graph for all steps (the parent commit captures one per step); a function that is wf_head
    above a sigma threshold and wf_row below re-captures exactly once. Final latents against the fp32 CPU oracle loop at the tiny-loop bar."""
    lat, captures = _graph_request(wf, gpu_device)
    base, _ = _graph_request(wf, gpu_device, fused=False)
    ref = _oracle_loop(wf)
    d, d0 = rel_l2(lat, ref), rel_l2(base, ref)
    print("tiny graph loop %s: captures %d, rel-L2 hip %.3e unfused-torch %.3e" % (name, captures, d, d0))
    assert captures == want_captures, captures
    assert d <= 1.5 * d0 + 2e-3 and d <= 2e-2, (d, d0)


def test_switch_function_really_switches():
    """(host only, but it belongs to the test above) the 4-step schedule of the tiny tools has sigmas on both sides of the threshold."""
    tools = cases.build_tools("tiny")
    sch = tools[4]
    sch.set_timesteps(4)
    sig = [float(s) for s in sch.sigmas[:4]]
    assert any(s > 3.0 for s in sig) and any(s <= 3.0 for s in sig), sig


def test_errors_touch_no_pointer(scope_lib, gpu_device):
    """Each unsupported / invalid call returns its documented code in front of any launch (the pointers here are not even mapped)."""
    from pww_hip._lib import AttnDesc, PWW_EINVAL, PWW_ENOTSUP
    lib = scope_lib
    P, null = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)

    def desc(M=77, D=40, N=256, H=8, B=2):
        d = AttnDesc()
        d.dtype, d.B, d.H, d.N, d.M, d.D = 0, B, H, N, M, D
        C = H * D
        d.q_stride[:] = [N * C, D, C]
        d.k_stride[:] = [0, D, C]
        d.v_stride[:] = [0, D, C]
        d.o_stride[:] = [N * C, D, C]
        d.scale = D ** -0.5
        d.bias_stride[:] = [0, 0, M, 1]
        return d

    def attn(d, kind=1, scope=1, parts=P, nparts=None):
        if nparts is None:
            nparts = lib.pww_scope_head_parts_count(ctypes.byref(d)) if scope == 1 else 0
        return lib.pww_scope_cross_attn_fwd(P, P, P, P, P, kind, scope, 1.0, null, ctypes.byref(d), parts, nparts, null, None, null)

    def parts(d, out=P, nbytes=1 << 30):
        return lib.pww_scope_head_parts(P, P, null, ctypes.byref(d), 1, out, nbytes, null)

    assert attn(desc(M=129), nparts=2) == PWW_ENOTSUP and attn(desc(M=129), scope=2, parts=null) == PWW_ENOTSUP and parts(desc(M=129)) == PWW_ENOTSUP
    assert attn(desc(D=12), nparts=2) == PWW_ENOTSUP and parts(desc(D=12)) == PWW_ENOTSUP
    assert attn(desc(), scope=0) == PWW_EINVAL
    assert attn(desc(M=1), kind=4, scope=2, parts=null) == PWW_EINVAL
    assert attn(desc(), parts=ctypes.c_void_p(0x10008)) == PWW_EINVAL and parts(desc(), out=ctypes.c_void_p(0x10008)) == PWW_EINVAL
    assert parts(desc(), nbytes=2 * 8 * 2 * 32 - 1) == PWW_EINVAL
    assert torch.cuda.is_available()
    torch.cuda.synchronize()      # nothing was launched, nothing faulted
