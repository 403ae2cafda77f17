"""Prompts longer than 77 tokens on the GPU: the launches of libpww_hip_long.so (128 < M <= 256 keys) call by call, and whole requests with a
160-token prompt encoded in three chunks.

Bars (none of them new):
  * per call against fp64 torch on the same rounded inputs: max|d| <= 2e-3 max|O| fp16 / 1.6e-2 max|O| bf16 (BASELINE.md
    section 4; gpu_util.TOL);
  * the folded statistics against pww_qk_reduce on the same Q: 1e-6 relative to the largest score (the header's statement for partials);
  * the new route against the three-launch route it replaces (pww_qk_reduce + general kernel with the map from HBM): two rounding steps of the
    storage type at the largest output, 2^-7 bf16 / 2^-10 fp16 of max|O| ("another rounding order of the same mathematics");
  * the probabilities launch: 4 x the fp32-torch error + 1e-6 against fp64 (tests/test_attn_maps_gpu.py);
  * final latents: rel-L2 <= 1e-2 fp16 / 5e-2 bf16 against the fp32 CPU run, and <= 1.5 x the unfused half-precision torch path on the same GPU + 2e-3;
    the modes among each other: 1e-2 (the existing loop tests' bar for two GPU runs); bf16 eager against folded / graph: 1.5 x the same pair on
    the 77-token path of the same GPU + 2e-3 (see test_long_request_three_modes_against_cpu_reference).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import pww_cases as cases
from gpu_util import TOL, install_unfused, uninstall_all, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def long_lib(gpu_device):
    """libpww_hip_long.so, built in-tree when missing (no conftest of its own: the module builds / locates the library itself)."""
    import build as pww_build
    path = pww_build.build_long()
    assert os.path.isfile(path)
    from pww_hip import _lib
    return _lib.load_long()


def _heads(t, H):
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H).permute(0, 2, 1, 3)


def _stat_value(st, kind, count):
    from pww_hip import ops
    st = st.double()
    if kind == ops.STAT_MAX:
        return st[:, 0]
    if kind == ops.STAT_STD:
        return ((st[:, 3] - st[:, 2] ** 2 / count) / (count - 1)).clamp_min(0).sqrt()
    return torch.ones_like(st[:, 0])


def _ref64(q, k, v, H, scale, w, c):
    """softmax((Q K^T + c[b] w) scale) V in fp64 on the rounded q / k / v; also the raw scores' per-image (max, min, sum, sum of squares)."""
    qh, kh, vh = _heads(q.double(), H), _heads(k.double(), H), _heads(v.double(), H)
    s = qh @ kh.transpose(-1, -2)
    st = torch.stack([s.amax((1, 2, 3)), s.amin((1, 2, 3)), s.sum((1, 2, 3)), (s * s).sum((1, 2, 3))], dim=1)
    return s, st, vh


def _apply(s, vh, scale, w, c):
    p = ((s + c.double().reshape(-1, 1, 1, 1) * w.double()) * scale).softmax(-1)
    o = p @ vh
    B, H, N, D = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, N, H * D)


def _map(N, M, cols, g, dev):
    """a dense [N, M] weight map whose non-zero columns are `cols` (regions: random row sets, strengths 0.2 .. 1.5)"""
    w = torch.zeros(N, M)
    for c in cols:
        rows = torch.rand(N, generator=g) < 0.3
        w[rows, c] = 0.2 + 1.3 * float(torch.rand((), generator=g))
    return w.to(dev)


MS = (154, 231, 129, 256)
NS = (4096, 1024, 256, 64, 4000)
DS = (40, 64, 80, 160)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M", MS)
def test_long_attention_per_call_parity(long_lib, gpu_device, dtype, M):
    """pww_long_qk_parts + pww_long_cross_attn_fwd_parts against fp64 torch, and against the three-launch route of the parent, over
    N x D x statistic x gate pattern x logit scale; maps with bias_cols in the second and the third chunk (and unknown)."""
    from pww_hip import ops
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(1000 + M)
    tol = TOL[dtype]
    tol_route = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    worst = {"fp64": 0.0, "route": 0.0, "stat": 0.0}
    case = 0
    for N in NS:
        for D in DS:
            H = 8 if (N >= 4000 and D == 40) or (N == 1024 and D == 80) or (N <= 256 and D == 160) else 2
            scale = D ** -0.5
            for std in (1.0, 4.0):
                for folded in (False, True):
                    case += 1
                    kind = (ops.STAT_MAX, ops.STAT_STD, ops.STAT_NONE)[case % 3]
                    B = 4 if folded else 2
                    amp = math.sqrt(std)
                    q = (torch.randn(B, N, H * D, generator=g) * amp).to(dev, dtype)
                    k = (torch.randn(1, M, H * D, generator=g) * amp).to(dev, dtype)
                    v = torch.randn(1, M, H * D, generator=g).to(dev, dtype)
                    # non-zero columns up to the second chunk / the third chunk / the map's last column (bound unknown)
                    variant = case // 3 % 3          # (independent of the statistic: case % 3)
                    last = min(M - 1, (140, 200, M - 1)[variant])
                    cols = sorted({3, 70, 100, last} if last > 100 else {3, 70, last})
                    w = _map(N, M, cols, g, dev)
                    bias_cols = 0 if variant == 2 else (last + 16) // 16 * 16
                    gate = torch.tensor([1.0, 1.0, 0.0, 0.0] if folded else [1.0, 1.0], device=dev)
                    gated = 2 if folded else 0
                    scalar = 0.9 if kind == ops.STAT_STD else 0.4 * math.log(1 + 7.84) if kind == ops.STAT_MAX else 3.0
                    tag = "M%d N%d D%d H%d %s std%g %s stat%d cols<%d" % (M, N, D, H, str(dtype)[6:], std, "folded" if folded else "all-1", kind, bias_cols)

                    parts = ops.long_qk_parts(q, k, H, kind, gate=gate, gated=gated) if kind != ops.STAT_NONE else None
                    stats_out = torch.zeros(B, 4, dtype=torch.float64, device=dev) if kind != ops.STAT_NONE else None
                    out = ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate, stat=(None, kind, scalar), parts=parts, stats_out=stats_out,
                                        bias_cols=bias_cols, gated=gated)
                    again = ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate, stat=(None, kind, scalar), parts=parts, bias_cols=bias_cols, gated=gated)
                    assert torch.equal(out, again), tag + ": two identical launches differ"

                    kx = k.expand(B, -1, -1)
                    s, st64, vh = _ref64(q, kx, v.expand(B, -1, -1), H, scale, w, None)
                    count = float(H * N * M)
                    c = torch.tensor(scalar, dtype=torch.float64, device=dev) * _stat_value(st64, kind, count) * gate.double()
                    ref = _apply(s, vh, scale, w, c)
                    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
                    worst["fp64"] = max(worst["fp64"], err)

                    # the statistics the attention launch folded, against pww_qk_reduce on the same Q (gated-in images)
                    serr = 0.0
                    if kind != ops.STAT_NONE:
                        st_red = ops.qk_stats(q, kx.contiguous(), H)
                        big = st_red[:, :2].abs().max().item()
                        live = gate != 0
                        if kind == ops.STAT_MAX:
                            serr = (stats_out[live, 0] - st_red[live, 0]).abs().max().item() / big
                        else:
                            serr = max((stats_out[live, 2] - st_red[live, 2]).abs().max().item() / (big * count),
                                       (stats_out[live, 3] - st_red[live, 3]).abs().max().item() / (big * big * count))
                        worst["stat"] = max(worst["stat"], serr)
                        # the route this replaces: pww_qk_reduce, then the general kernel reading the map score by score
                        old = ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate, stat=(st_red, kind, scalar))
                    else:
                        old = ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate * scalar)
                    rerr = (out.double() - old.double()).abs().max().item() / old.double().abs().max().item()
                    worst["route"] = max(worst["route"], rerr)
                    print("%s: vs fp64 %.3e (bar %.1e)  vs three-launch route %.3e (bar %.2e)  stats %.2e" % (tag, err, tol, rerr, tol_route, serr))
                    assert err <= tol, (tag, err)
                    assert serr <= 1e-6, (tag, serr)
                    assert rerr <= tol_route, (tag, rerr)
    print("M%d %s worst: %s" % (M, str(dtype)[6:], worst))


def _probs_ref(q, k, H, scale, bias, c, dt):
    s = _heads(q.to(dt), H) @ _heads(k.to(dt), H).transpose(-1, -2)
    if bias is not None:
        s = s + c.to(dt).reshape(-1, 1, 1, 1) * bias.to(dt)
    return (s * scale).softmax(-1).mean(1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_long_probs_vs_fp64(long_lib, gpu_device, dtype):
    """pww_long_cross_attn_probs: 4 x the fp32-torch error + 1e-6 against fp64; row sums equal `weight`; padding and images past `images`
    untouched; two identical calls give identical bits."""
    from pww_hip import ops
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(21)
    case = 0
    for (H, N, D) in [(8, 4096, 40), (8, 1024, 80), (8, 256, 160), (8, 64, 160), (5, 1000, 64)]:
        for M in ((231,) if N >= 4000 else (154, 231, 129, 256)):
            for std in (1.0, 4.0):
                case += 1
                B, scale = 3, D ** -0.5
                amp = math.sqrt(std)
                q = (torch.randn(B, N, H * D, generator=g) * amp).to(dev, dtype)
                k = (torch.randn(B, M, H * D, generator=g) * amp).to(dev, dtype)
                w = ((torch.rand(N, M, generator=g) < 0.15).float() * torch.rand(N, M, generator=g) * 1.5).to(dev)
                gate = torch.tensor([1.0, 0.0, 1.0], device=dev)
                st = ops.qk_stats(q, k, H)
                kind = (ops.STAT_MAX, ops.STAT_STD, ops.STAT_NONE)[case % 3]
                scalar = 0.4 * math.log(1 + 7.84) if kind != ops.STAT_STD else 0.9
                c = (torch.tensor(scalar, dtype=torch.float32, device=dev) * _stat_value(st, kind, float(H * N * M)).float()) * gate
                weight = (1.0, 0.25)[case % 2]
                poison = 1234.5
                pad = (M + 3) // 4 * 4 + 4
                store = torch.full((B, N, pad), poison, device=dev)
                out = store[:, :, :M]
                ops.attention_probs(q, k, H, scale, bias=w, bias_coeff=gate, stat=(st if kind != ops.STAT_NONE else None, kind, scalar), images=2, out=out, weight=weight)
                r64 = _probs_ref(q, k, H, scale, w, c, torch.float64)[:2] * weight
                r32 = _probs_ref(q, k, H, scale, w, c, torch.float32)[:2].double() * weight
                err, yard = (out[:2].double() - r64).abs().max().item(), (r32 - r64).abs().max().item()
                sums = (out[:2].sum(-1) - weight).abs().max().item()
                print("H%d N%d D%d M%d %s std%g stat%d: max abs err %.3e, fp32 torch %.3e; max |row sum - weight| %.3e" % (H, N, D, M, str(dtype)[6:], std, kind, err, yard, sums))
                assert err <= 4 * yard + 1e-6
                assert sums <= 1e-5          # (the bar of tests/test_attn_maps_gpu.py)
                assert bool((store[2] == poison).all()) and bool((store[:, :, M:] == poison).all())
                again = torch.full((B, N, pad), poison, device=dev)
                ops.attention_probs(q, k, H, scale, bias=w, bias_coeff=gate, stat=(st if kind != ops.STAT_NONE else None, kind, scalar), images=2, out=again[:, :, :M], weight=weight)
                assert torch.equal(store, again)


# ---- whole requests: a 160-token prompt whose regions sit in chunks 1, 2 and 3 ---------------------------------------------------------------
def _long_case(shift=0, size=512):
    """3 vertical stripes (cases.stripes_case) painted with phrases at content positions 5 + shift, 90 + shift and 155 of a 160-token prompt."""
    img, ctx, _ = cases.stripes_case(3, size)
    words = [v.split(",")[0] for v in ctx.values()]
    toks = ["filler%d" % (i + 1000 * shift) for i in range(160)]
    for w, pos in zip(words, (5 + shift, 90 + shift, 155)):
        toks[pos] = w
    ctx = {color: v.split(",")[0] + ",1.0" for color, v in ctx.items()}
    return img, ctx, " ".join(toks), words


def _request(mode, tools, device, case, chunks, wf, steps=10, seed=3, record=False, unfused=False):
    import importlib
    import pww_hip
    import paint_with_words as pw
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    img, ctx, prompt = case[:3]
    kw = dict(color_context=dict(ctx), color_map_image=Image.fromarray(img), input_prompt=prompt, num_inference_steps=steps, guidance_scale=7.5,
              seed=seed, device=str(device), weight_function=wf, preloaded_utils=tools, return_latents=True, max_prompt_chunks=chunks)
    old = pww_mod.DEFAULT_MODE
    pww_mod.DEFAULT_MODE = mode
    from pww_hip import sampler as S
    orig_install = S.install
    if unfused:
        S.install = install_unfused
    try:
        if not record:
            return pw.paint_with_words(**kw).clone(), None
        with pww_hip.record_attention_maps() as rec:
            lat = pw.paint_with_words(**kw).clone()
        return lat, rec.maps()
    finally:
        S.install = orig_install
        pww_mod.DEFAULT_MODE = old


def _cpu_reference(case, wf, steps, seed):
    """fp32 CPU run of the same request from oracle.pww_oracle's functions, fed the [1, 231, ctx] context and [N, 231] maps. The oracle's
    encode_text_color_inputs tokenizes to 77; its lines are restated here for three chunks: phrases matched on the unframed ids
    (tokens_img_attention_weight), columns scattered to 1 + p + 2 (p // 75), every chunk through the text encoder on its own."""
    from oracle import pww_oracle as O
    img, ctx, prompt = case[:3]
    vae, unet, text, tok, sch = cases.build_tools("tiny")
    per = tok.model_max_length - 2
    content = list(tok(prompt, max_length=1 << 20, truncation=False)["input_ids"][1:-1])
    k = -(-len(content) // per)
    assert k == 3
    bos, eos = tok("")["input_ids"][:2]
    rows = [[bos] + content[j * per:(j + 1) * per] for j in range(k)]
    rows = [r + [eos] * (per + 2 - len(r)) for r in rows]
    color_context, extra_seeds, _ = O.extract_seed_and_sigma(dict(ctx))
    regions, width, height = O.separate_regions(img, color_context, tok)
    col = [1 + p + 2 * (p // per) for p in range(len(content))]

    def framed(w):      # [..., content] -> [..., 77 k]
        out = np.zeros(w.shape[:-1] + (k * (per + 2),), dtype=np.float32)
        out[..., col] = w
        return torch.from_numpy(out)

    encode = lambda rs: torch.cat([text(torch.tensor([r]))[0] for r in rs], dim=1)      # noqa: E731
    cond = {"CONTEXT_TENSOR": encode(rows), "CROSS_ATTENTION_WEIGHT_ORIG": framed(O.tokens_img_attention_weight(regions, content, 1, True))}
    uncond = {"CONTEXT_TENSOR": encode([[bos] + [eos] * (per + 1)] * k), "CROSS_ATTENTION_WEIGHT_ORIG": 0}
    for r in (8, 16, 32, 64):
        key = f"CROSS_ATTENTION_WEIGHT_{O.always_round(height / r) * O.always_round(width / r)}"
        cond[key] = framed(O.tokens_img_attention_weight(regions, content, r))
        uncond[key] = 0
    O.install_oracle_attention(unet)
    try:
        latents = O.initial_latents(seed, unet.in_channels, img.shape[0], img.shape[1], regions, extra_seeds)
        return O.sample_latents(unet, sch, cond, uncond, latents, steps, 7.5, wf), cond
    finally:
        uninstall_all()


def test_short_prompt_with_cap_three_gives_todays_context(long_lib, gpu_device):
    """A prompt of at most 75 tokens with max_prompt_chunks=3: the same context dicts as the default call, bit for bit."""
    from pww_hip import conditioning as C
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    img = Image.fromarray(cases.load_example_rgb())
    outs = []
    for chunks in (1, 3):
        outs.append(C._encode_text_color_inputs(tools[2], tools[3], gpu_device, img, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "", dtype=torch.float16,
                                                max_prompt_chunks=chunks))
    for a, b in ((outs[0][2], outs[1][2]), (outs[0][3], outs[1][3])):
        assert sorted(dict.keys(a)) == sorted(dict.keys(b))
        for key in dict.keys(a):
            if torch.is_tensor(a[key]):
                assert a[key].shape == b[key].shape and torch.equal(a[key], b[key]), key
            else:
                assert a[key] == b[key], key
    assert outs[0][2]["CONTEXT_TENSOR"].shape[1] == 77


class _LaunchCounts:
    """Counts, while active, the launches of ops.attention's bias routes: the long pair against the three-launch route it replaces
    (pww_qk_reduce + the general kernel: `stat` / `reduce`) and the <= 128-key pass-2-only launch (`parts`)."""
    NAMES = (("_launch_long", "long"), ("_launch_stat", "stat"), ("_launch_parts", "parts"), ("qk_stats", "reduce"), ("long_qk_parts", "long_parts"))

    def __enter__(self):
        from pww_hip import ops
        self.n = {key: 0 for _, key in self.NAMES}
        self._real = {name: getattr(ops, name) for name, _ in self.NAMES}
        for name, key in self.NAMES:
            def f(*a, _name=name, _key=key, **kw):
                self.n[_key] += 1
                return self._real[_name](*a, **kw)
            setattr(ops, name, f)
        return self

    def __exit__(self, *exc):
        from pww_hip import ops
        for name, f in self._real.items():
            setattr(ops, name, f)
        return False


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_long_request_three_modes_against_cpu_reference(long_lib, gpu_device, dtype):
    """Tiny UNet, 10 LMS steps, 160-token prompt with regions in chunks 1, 2 and 3, fp16 and bf16: eager, folded and graph mode agree with the
    fp32 CPU run and stay within 1.5 x the unfused half-precision torch path + 2e-3; they agree with each other; the long route serves every
    cross-attention call that carries a map in ALL three modes; a second request with another 160-token prompt replays the captured graph,
    a request with another chunk count re-captures.

    Agreement between the modes. fp16: 1e-2, the bar tests/test_loop_gpu.py and tests/test_attn_maps_gpu.py hold two GPU runs of one request
    to. Folded and graph mode run the same kernels on the same batch: 1e-2 in bf16 as well. Eager mode evaluates the UNet as two batch-1
    calls where folded / graph mode make one batch-2 call: the stock GEMM / convolution kernels round differently per batch size, and in
    bf16 (8 significant bits) ten steps of that do not stay inside the fp16 bar -- on the 77-token path too, which this change does not touch.
    No existing test compares two bf16 runs, so the yardstick is that path: the same request with max_prompt_chunks=1 on the same GPU, the same
    pair of modes, and the project's form for a bar relative to a yardstick (tests/test_loop_gpu.py): <= 1.5 x yardstick + 2e-3. Every figure
    is printed before it is asserted. Measured on an MI355X: fp16 eager vs folded / graph 2.08e-3 (77-token path 2.01e-3), bf16 1.49e-2
    (77-token path 1.43e-2); folded vs graph 0 in both dtypes."""
    dev = gpu_device
    steps, seed, wf = 10, 3, cases.weight_fn_runner
    bar = 1e-2 if dtype == torch.float16 else 5e-2
    name = str(dtype)[6:]
    case = _long_case()
    ref, cond_ref = _cpu_reference(case, wf, steps, seed)
    assert cond_ref["CONTEXT_TENSOR"].shape[1] == 231
    try:
        tools = cases.build_tools("tiny", dtype=dtype, device=dev)
        n_cross = sum(1 for nm, _ in tools[1].named_modules() if nm.endswith("attn2"))
        lat = {}
        for mode in ("eager", "folded", "graph"):
            with _LaunchCounts() as c:
                lat[mode] = _request(mode, tools, dev, case, 3, wf, steps, seed)[0]
            print("%s %s: launches %s (%d cross-attention layers x %d steps)" % (name, mode, c.n, n_cross, steps))
            # eager: one conditional batch-1 call per layer and step; folded: one folded call per layer and step; graph: the calls of the captures
            assert c.n["long"] == c.n["long_parts"] and c.n["stat"] == c.n["parts"] == c.n["reduce"] == 0, (mode, c.n)
            if mode == "graph":
                assert c.n["long"] >= n_cross and c.n["long"] % n_cross == 0, c.n
            else:
                assert c.n["long"] == n_cross * steps, (mode, c.n)
        sampler = tools[1]._pww_samplers[(id(tools[4]), "graph")]
        before = sampler._graphed.captures
        base = _request("eager", tools, dev, case, 3, wf, steps, seed, unfused=True)[0]
        d0 = rel_l2(base, ref)
        for mode, l in lat.items():
            d = rel_l2(l, ref)
            print("%s %s: final-latent rel-L2 vs fp32 CPU %.3e (bar %.0e), unfused torch %.3e" % (name, mode, d, bar, d0))
        for mode, l in lat.items():
            d = rel_l2(l, ref)
            assert d <= bar and d <= 1.5 * d0 + 2e-3, (mode, d, d0)

        # a second request with another 160-token prompt replays the captured graph
        other = _long_case(shift=2)
        l2 = _request("graph", tools, dev, other, 3, wf, steps, seed)[0]
        assert sampler._graphed.captures == before, "another 160-token prompt re-captured the graph"
        l2_f = _request("folded", tools, dev, other, 3, wf, steps, seed)[0]
        d_replay = rel_l2(l2, l2_f)
        print("%s replayed graph vs folded, second prompt: rel-L2 %.3e" % (name, d_replay))
        assert d_replay <= 1e-2 and rel_l2(l2, lat["graph"]) > 1e-3

        # the yardstick of the mode pairs: the same request on the 77-token path (max_prompt_chunks=1); in graph mode another k re-captures
        short = {}
        for mode in ("eager", "folded", "graph"):
            with _LaunchCounts() as c:
                short[mode] = _request(mode, tools, dev, case, 1, wf, steps, seed)[0]
            assert c.n["long"] == 0, (mode, c.n)
        assert sampler._graphed.captures > before
        pairs = (("eager", "folded"), ("eager", "graph"), ("folded", "graph"))
        got = {ab: rel_l2(lat[ab[0]], lat[ab[1]]) for ab in pairs}
        yard = {ab: rel_l2(short[ab[0]], short[ab[1]]) for ab in pairs}
        for ab in pairs:
            print("%s %s vs %s: rel-L2 %.3e (the 77-token path, same modes: %.3e)" % (name, ab[0], ab[1], got[ab], yard[ab]))
        for ab in pairs:
            if dtype == torch.float16 or ab == ("folded", "graph"):
                assert got[ab] <= 1e-2, (ab, got[ab])
            else:
                assert got[ab] <= 1.5 * yard[ab] + 2e-3, (ab, got[ab], yard[ab])
    finally:
        uninstall_all()


def test_phrase_in_the_second_chunk_needs_the_cap(long_lib, gpu_device):
    """The feature from the outside: the same request with cap 1 and cap 3. With cap 1 the phrase of the second chunk is cut off the prompt
    (no map); with cap 3 its recorded map is brighter inside its painted stripe than outside (a sign condition)."""
    from pww_hip._lib import PwwHipError
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device)
    case = _long_case()
    words = case[3]
    wf = lambda w, sigma, qk: 5 * w * math.log(1 + sigma) * qk.max()          # noqa: E731
    try:
        _, maps1 = _request("folded", tools, gpu_device, case, 1, wf, steps=4, record=True)
        assert maps1.tokens().shape[1] == 77
        maps1.phrase(words[0])
        for w in words[1:]:
            with pytest.raises(PwwHipError, match="does not occur"):
                maps1.phrase(w)
        _, maps3 = _request("folded", tools, gpu_device, case, 3, wf, steps=4, record=True)
        assert maps3.tokens().shape[1] == 231
        H, W = max(maps3.resolutions.values())
        for i, w in enumerate(words):
            m = maps3.phrase(w)[0]
            inside = torch.zeros(H, W, dtype=torch.bool, device=m.device)
            inside[:, i * W // 3:(i + 1) * W // 3] = True
            mi, mo = m[inside].mean().item(), m[~inside].mean().item()
            print("%s (chunk %d): inside %.4f outside %.4f" % (w, i + 1, mi, mo))
            assert mi > mo, (w, mi, mo)
        assert maps3.columns(words[1]) == [1 + 90 + 2] and maps3.columns(words[2]) == [1 + 155 + 4]
    finally:
        uninstall_all()
