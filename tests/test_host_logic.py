"""CPU tests of the host logic and the C-ABI boundary (no compute calls: there is no GPU here)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import pww_cases as cases
from oracle import pww_oracle as O


def test_library_loads_and_exports_every_declared_symbol(built_lib):
    """libpww_hip.so exports exactly what include/pww_hip.h declares outside its "experiments" section -- and none of the experiments
    section (the product library holds the default routes and the documented switches, nothing else)."""
    import pww_hip
    from pww_hip import _lib
    lib = pww_hip.load_library()
    header = open(os.path.join(cases.REPO, "include", "pww_hip.h")).read()
    cut = header.index("= experiments =")
    code = lambda text: re.sub(r"/\*.*?\*/", " ", text, flags=re.S)       # noqa: E731  (declarations only: comments name functions too)
    product = set(re.findall(r"\b(pww_[a-z0-9_]+)\s*\(", code(header[:cut] + "*/")))
    moved = set(re.findall(r"\b(pww_[a-z0-9_]+)\s*\(", code("/*" + header[cut:])))
    assert product == set(pww_hip.EXPORTS), product ^ set(pww_hip.EXPORTS)
    assert moved == set(_lib.EXPERIMENT_EXPORTS), moved ^ set(_lib.EXPERIMENT_EXPORTS)
    raw = ctypes.CDLL(built_lib)
    for name in product:
        assert hasattr(raw, name), name
    for name in moved:
        assert not hasattr(raw, name), "%s belongs to libpww_hip_experiments.so" % name
    assert lib.pww_version() == 127 and lib.pww_has_experiments() == 0 and not _lib.has_experiments()
    assert lib.pww_last_error() == b"" or isinstance(lib.pww_last_error(), bytes)
    assert lib.pww_workspace_bytes(None) == 0
    assert os.path.getsize(built_lib) <= 6 * 1024 * 1024, "the product library grew past 6 MB: %d bytes" % os.path.getsize(built_lib)


def test_experiments_library_is_a_superset(experiments_lib):
    """libpww_hip_experiments.so (tests / tools only; built by the `experiments_lib` fixture when missing): every product symbol plus the
    header's experiments section, same ABI version, and it says what it is."""
    from pww_hip import _lib
    raw = ctypes.CDLL(experiments_lib)
    for name in _lib.EXPORTS + _lib.EXPERIMENT_EXPORTS:
        assert hasattr(raw, name), name
    raw.pww_has_experiments.restype = ctypes.c_int
    assert raw.pww_has_experiments() == 1 and raw.pww_version() == 127
    assert _lib.load_experiments().pww_has_experiments() == 1


def test_struct_layout_matches_header():
    from pww_hip._lib import AttnDesc, Region
    assert ctypes.sizeof(Region) == 8
    # int32 x6, int64 x12, float (+pad), int64 x4
    assert ctypes.sizeof(AttnDesc) == 24 + 96 + 8 + 32
    assert AttnDesc.q_stride.offset == 24 and AttnDesc.scale.offset == 120 and AttnDesc.bias_stride.offset == 128
    # pww_cross_opts_t: uint32 size, int32 bias_cols, 3 pointers, int32 R, int32 gated_images (padding before ABI 1.21), int64 x3
    from pww_hip._lib import CrossOpts
    assert ctypes.sizeof(CrossOpts) == 64
    assert (CrossOpts.bias_cols.offset, CrossOpts.coeff_scalar_dev.offset, CrossOpts.col_idx.offset, CrossOpts.R.offset,
            CrossOpts.gated_images.offset, CrossOpts.compact_stride.offset, CrossOpts.col_idx_stride.offset) == (4, 8, 24, 32, 36, 40, 56)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pww_hip.h")).read()
    body = header[header.index("typedef struct pww_cross_opts {"):header.index("} pww_cross_opts_t;")]
    assert [m for m in re.findall(r"\b(\w+)(?:\[\d+\])?;", body)] == ["size", "bias_cols", "coeff_scalar_dev", "bias_compact", "col_idx", "R", "gated_images",
                                                                    "compact_stride", "col_idx_stride"]


def test_no_cpu_fallback():
    """The product path refuses CPU tensors instead of silently computing somewhere else."""
    import pww_hip
    from pww_hip import ops
    x = torch.randn(1, 32, 64).half()
    with pytest.raises(pww_hip.PwwHipError):
        ops.attention(x, x, x, 2, 1.0)
    with pytest.raises(pww_hip.PwwHipError):
        ops.qk_stats(x, x, 2)
    from sd_standin import CrossAttention
    mod = CrossAttention(64, None, 2, 32)
    with pytest.raises(pww_hip.PwwHipError):
        pww_hip.inj_forward(mod, torch.randn(1, 32, 64))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    import pww_hip._lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(L.PwwHipError, match="no CPU/PyTorch fallback"):
        L.load()


def test_product_does_not_import_oracle():
    pkg = os.path.join(cases.REPO, "paint-with-words-sd_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(root, f)


def test_host_parsers_match_reference_kats():
    from pww_hip import conditioning as C
    kat = json.load(open(os.path.join(cases.GOLDEN, "kat.json")))
    for x, y in kat["always_round"]:
        assert C.always_round(x) == y
    for case in kat["extract"]:
        ctx = dict(case["input"])
        out, seeds, sigmas = C._extract_seed_and_sigma_from_context(ctx)
        assert dict(out) == case["output"] and ctx == case["output"]
        assert {str(k): v for k, v in seeds.items()} == case["seeds"]
        assert {str(k): v for k, v in sigmas.items()} == case["sigmas"]
    with pytest.raises(ValueError):   # 3 fields, last two not integers
        C._extract_seed_and_sigma_from_context({"a": "x,1.0,abc"})


def test_column_lists_match_oracle(capsys):
    from pww_hip import conditioning as C
    from sd_standin import HashTokenizer
    tok = HashTokenizer()
    prompt = cases.RUNNER_PROMPT + " dog"
    ids = tok([prompt], padding="max_length", max_length=77, truncation=True, return_tensors="pt")["input_ids"][0].tolist()
    ctx = dict(cases.RUNNER_CONTEXT)
    ctx["#0a0b0c"] = "sandy ground,0.7"      # hex colour key + multi-token phrase overlapping "ground"
    ctx[(9, 9, 9)] = "unicorn,1.0"           # phrase not in the prompt -> warning only
    table = C._parse_regions(ctx, tok)
    assert table[5][1] == (10, 11, 12)
    regions, _, _ = O.separate_regions(np.zeros((8, 8, 3), np.uint8), dict(ctx), tok)
    assert C._column_lists(table, ids) == O.column_region_lists(regions, ids)
    assert "not found in text" in capsys.readouterr().out


def test_schedulers():
    from sd_standin import LMSDiscreteScheduler, PLMSScheduler
    s = LMSDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    assert abs(float(s.init_noise_sigma) - 14.6146) < 1e-3
    s.set_timesteps(10)
    assert s.timesteps.tolist() == [999.0, 888.0, 777.0, 666.0, 555.0, 444.0, 333.0, 222.0, 111.0, 0.0]
    assert abs(float(s.sigmas[1]) - 7.8399) < 1e-3 and float(s.sigmas[-1]) == 0.0
    x = torch.ones(1, 4, 2, 2)
    assert torch.allclose(s.scale_model_input(x, s.timesteps[0]), x / (14.6146 ** 2 + 1) ** 0.5, atol=1e-5)
    p = PLMSScheduler()
    p.set_timesteps(30)
    ts = p.timesteps.tolist()
    assert len(ts) == 31 and ts[:4] == [958, 925, 925, 892] and ts[-1] == 1
    ac = p.alphas_cumprod[958]
    assert abs(float(p.sigmas[0]) - float(((1 - ac) / ac) ** 0.5)) < 1e-6
    # PLMS on a linear "model" reproduces the exact solution path ordering (finite, monotone sample norm decay)
    lat = torch.ones(1, 4, 2, 2)
    for t in p.timesteps:
        lat = p.step(0.1 * lat, t, lat).prev_sample
    assert torch.isfinite(lat).all()


def test_qk_proxy_reductions_with_injected_stats(monkeypatch):
    """QKProxy maths (max/min/mean/std/abs().max, per-image shapes) with the kernel call replaced by a
    CPU computation of the same statistics -- the kernel itself is checked on the GPU."""
    from pww_hip import attention as A
    B, H, N, M, D = 2, 3, 10, 7, 8
    q, k = torch.randn(B, N, H * D), torch.randn(B, M, H * D)
    scores = torch.matmul(O.split_heads(q, H), O.split_heads(k, H).transpose(-1, -2)).reshape(B, -1).double()

    def fake_stats(q_, k_, heads):
        return torch.stack([scores.max(1).values, scores.min(1).values, scores.sum(1), (scores ** 2).sum(1)], 1)
    monkeypatch.setattr(A.ops, "qk_stats", fake_stats)
    p = A.QKProxy(q, k, H)
    assert p.shape == (B * H, N, M)
    assert p.max().shape == (B, 1, 1, 1)
    assert torch.allclose(p.max().flatten(), scores.max(1).values.float())
    assert torch.allclose(p.std().flatten(), scores.std(1).float(), rtol=1e-5)
    assert torch.allclose(p.mean().flatten(), scores.mean(1).float(), atol=1e-6)
    assert torch.allclose(p.abs().max().flatten(), scores.abs().max(1).values.float())
    p1 = A.QKProxy(q[:1], k[:1], H)
    monkeypatch.setattr(A.ops, "qk_stats", lambda *a: fake_stats(*a)[:1])
    assert p1.max().dim() == 0                       # batch 1: a 0-dim tensor, like torch's qk.max()
    bias = cases.weight_fn_runner(torch.ones(N, M), torch.tensor(3.0), p1)
    assert bias.shape == (N, M)


def test_lazy_stat_algebra(monkeypatch):
    """LazyStat (symbolic scale * reduce(qk)): Python factors stay symbolic and reach the kernel call as
    (stats, kind, scalar); anything else materialises the tensor the old path produced."""
    from pww_hip import attention as A
    B, H, N, M, D = 2, 2, 6, 5, 8
    q, k = torch.randn(B, N, H * D), torch.randn(B, M, H * D)
    scores = torch.matmul(O.split_heads(q, H), O.split_heads(k, H).transpose(-1, -2)).reshape(B, -1).double()
    monkeypatch.setattr(A.ops, "qk_stats", lambda q_, k_, h: torch.stack(
        [scores.max(1).values, scores.min(1).values, scores.sum(1), (scores ** 2).sum(1)], 1))
    p = A.QKProxy(q, k, H)
    w = torch.rand(N, M)
    for fn, kind, ref in ((cases.weight_fn_runner, A.ops.STAT_MAX, scores.max(1).values),
                          (cases.weight_fn_std, A.ops.STAT_STD, scores.std(1))):
        r = fn(A.ScaledW(w), torch.tensor(7.0), p)
        assert isinstance(r, A.ScaledW) and r.w is w and isinstance(r.stat, A.LazyStat) and r.stat.kind == kind
        want = fn(w.expand(B, 1, N, M), torch.tensor(7.0), type("Q", (), {"max": lambda s: ref.float().reshape(B, 1, 1, 1),
                                                                          "std": lambda s: ref.float().reshape(B, 1, 1, 1)})())
        assert torch.allclose(r.materialize(), want, rtol=1e-5)
    s = 2.0 * p.max() / 4.0
    assert isinstance(s, A.LazyStat) and s.scale == 0.5
    assert torch.allclose(s.materialize().flatten(), 0.5 * scores.max(1).values.float())
    assert isinstance(-p.min(), A.LazyStat) and torch.allclose((-p.min()).materialize().flatten(), -scores.min(1).values.float())
    # tensor arithmetic, torch functions and comparisons fall back to real tensors
    assert torch.is_tensor(p.max() + 1.0) and torch.is_tensor(torch.exp(p.mean())) and torch.is_tensor(p.max() * torch.ones(1))
    assert bool((p.max() >= p.min()).all()) and p.max().shape == (B, 1, 1, 1)
    r2 = (A.ScaledW(w) * p.max()) * p.std()          # two statistics: second one goes through tensors
    assert isinstance(r2, A.ScaledW) and r2.stat is None
    assert torch.allclose(r2.materialize(), w * scores.max(1).values.float().reshape(B, 1, 1, 1) * scores.std(1).float().reshape(B, 1, 1, 1), rtol=1e-5)


def test_miopen_find_switch(monkeypatch):
    """enable_miopen_find(): on by default, off with PWW_MIOPEN_FIND=0 (what conftest.py sets for the parity tests)."""
    import pww_hip
    old = torch.backends.cudnn.benchmark
    try:
        torch.backends.cudnn.benchmark = False
        monkeypatch.setenv("PWW_MIOPEN_FIND", "0")
        pww_hip.enable_miopen_find()
        assert torch.backends.cudnn.benchmark is False
        monkeypatch.setenv("PWW_MIOPEN_FIND", "1")
        pww_hip.enable_miopen_find()
        assert torch.backends.cudnn.benchmark is True
        torch.backends.cudnn.benchmark = False
        monkeypatch.delenv("PWW_MIOPEN_FIND")
        pww_hip.enable_miopen_find()
        assert torch.backends.cudnn.benchmark is True
        # the scoped form the drop-in API uses: on inside, the caller's value restored afterwards (no global side effect)
        torch.backends.cudnn.benchmark = False
        with pww_hip.miopen_find():
            assert torch.backends.cudnn.benchmark is True
        assert torch.backends.cudnn.benchmark is False
        monkeypatch.setenv("PWW_MIOPEN_FIND", "0")
        with pww_hip.miopen_find():
            assert torch.backends.cudnn.benchmark is False
    finally:
        torch.backends.cudnn.benchmark = old


def test_scaled_w_algebra():
    """ScaledW (lazy coeff * w): scalar / per-image factors fold into the coefficient, anything else falls back to
    the real tensor with identical values."""
    from pww_hip.attention import ScaledW
    w = torch.rand(6, 5)
    qmax1, qmaxB = torch.tensor(3.0), torch.tensor([2.0, 4.0]).reshape(2, 1, 1, 1)
    r = 0.4 * ScaledW(w) * math.log(1 + 7.0) * qmax1
    assert isinstance(r, ScaledW) and r.w is w
    assert torch.allclose(r.materialize(), 0.4 * w * math.log(8.0) * qmax1)
    rb = cases.weight_fn_runner(ScaledW(w), torch.tensor(7.0), type("Q", (), {"max": lambda self: qmaxB})())
    assert isinstance(rb, ScaledW) and rb.coeff.shape == (2, 1, 1, 1)
    assert torch.allclose(rb.materialize(), cases.weight_fn_runner(w, torch.tensor(7.0), type("Q", (), {"max": lambda self: qmaxB})()))
    assert isinstance(ScaledW(w) / 2.0, ScaledW) and torch.allclose((ScaledW(w) / 2.0).materialize(), w / 2)
    # non-linear uses materialise
    assert torch.is_tensor(ScaledW(w, 2.0) + 1.0) and torch.allclose(ScaledW(w, 2.0) + 1.0, 2 * w + 1)
    assert torch.allclose(torch.tanh(ScaledW(w, 2.0)), torch.tanh(2 * w))
    assert torch.allclose(ScaledW(w, 2.0) * torch.ones(6, 5), 2 * w)
    assert ScaledW(w, 2.0).shape == w.shape and torch.allclose(ScaledW(w, 3.0)[1], 3 * w[1])
    assert torch.allclose((ScaledW(w, 2.0) ** 2), (2 * w) ** 2) and torch.allclose(1.0 - ScaledW(w), 1.0 - w)


def test_public_api_matches_reference_signatures():
    """Drop-in surface: what runner.py / runner_inpaint.py import must exist, and the function API must take the
    reference's parameters with the reference's defaults (paint_with_words.py:393-413, :128-140;
    paint_with_words_inpaint.py:139-157). Extra keyword-only-in-practice extensions must come last."""
    import inspect
    import paint_with_words as pw
    from paint_with_words import (paint_with_words, PaintWithWord_StableDiffusionPipeline,            # runner.py:7
                                  paint_with_words_inpaint, PaintWithWord_StableDiffusionInpaintPipeline,  # runner_inpaint.py:6
                                  pww_load_tools, fig_from_settings)                                  # __init__.py:1-3
    sig = inspect.signature(paint_with_words)
    ref = [("color_context", {}), ("color_map_image", None), ("input_prompt", ""), ("num_inference_steps", 30),
           ("guidance_scale", 7.5), ("seed", 0), ("scheduler_type", None), ("device", "cuda:0"), ("weight_function", None),
           ("local_model_path", None), ("hf_model_path", "CompVis/stable-diffusion-v1-4"), ("preloaded_utils", None),
           ("unconditional_input_prompt", ""), ("model_token", None), ("init_image", None), ("strength", 0.5)]
    names = list(sig.parameters)
    assert names[: len(ref)] == [n for n, _ in ref]
    for n, dflt in ref:
        if n not in ("scheduler_type", "weight_function"):
            assert sig.parameters[n].default == dflt, n
    assert sig.parameters["scheduler_type"].default.__name__ == "LMSDiscreteScheduler"
    wf = sig.parameters["weight_function"].default                       # 0.1 * w * log(sigma + 1) * qk.max()
    assert abs(float(wf(torch.tensor(2.0), torch.tensor(3.0), torch.tensor([1.0, 5.0]))) - 0.1 * 2 * math.log(4.0) * 5) < 1e-6
    sig_i = inspect.signature(paint_with_words_inpaint)
    ref_i = ["color_context", "color_map_image", "mask_image", "init_image", "input_prompt", "num_inference_steps", "guidance_scale",
             "seed", "scheduler_type", "device", "weight_function", "local_model_path", "hf_model_path", "preloaded_utils",
             "unconditional_input_prompt", "model_token", "strength"]
    assert list(sig_i.parameters)[: len(ref_i)] == ref_i
    assert sig_i.parameters["num_inference_steps"].default == 150 and sig_i.parameters["strength"].default == 1.0
    assert sig_i.parameters["hf_model_path"].default == "runwayml/stable-diffusion-inpainting"
    assert list(inspect.signature(pww_load_tools).parameters) == ["device", "scheduler_type", "local_model_path", "hf_model_path", "model_token"]
    assert list(inspect.signature(pw.inj_forward).parameters) == ["self", "hidden_states", "context", "mask"]
    with pytest.raises(AssertionError):
        pww_load_tools(device="cpu")          # reference :142-144: a model path is required


def test_pipeline_call_signatures_match_reference():
    """The pipeline classes take the reference's parameters in the reference's ORDER with its defaults
    (paint_with_words.py:631-655, paint_with_words_inpaint.py:341-361): positional callers and `image=` / `eta=` users
    of the reference land on the same arguments here."""
    import inspect
    from paint_with_words import PaintWithWord_StableDiffusionPipeline as P, PaintWithWord_StableDiffusionInpaintPipeline as PI
    ref = [("self", None), ("prompt", None), ("color_map_image", None), ("color_context", {}), ("weight_function", "f"), ("height", None), ("width", None),
           ("num_inference_steps", 30), ("guidance_scale", 7.5), ("negative_prompt", ""), ("num_images_per_prompt", 1), ("eta", 0.5), ("seed", 0),
           ("generator", None), ("image", None), ("latents", None), ("output_type", "pil"), ("return_dict", True), ("callback", None), ("callback_steps", 1)]
    params = inspect.signature(P.__call__).parameters
    assert list(params) == [n for n, _ in ref]
    for n, d in ref[2:]:
        if d != "f":
            assert params[n].default == d, n
    ref_i = [("self", None), ("prompt", None), ("image", None), ("mask_image", None), ("color_map_image", None), ("color_context", {}), ("weight_function", "f"),
             ("height", None), ("width", None), ("num_inference_steps", 30), ("guidance_scale", 7.5), ("negative_prompt", ""), ("num_images_per_prompt", 1),
             ("eta", 1.0), ("seed", 0), ("generator", None), ("latents", None), ("output_type", "pil"), ("return_dict", True), ("callback", None), ("callback_steps", 1)]
    params = inspect.signature(PI.__call__).parameters
    assert list(params) == [n for n, _ in ref_i]
    for n, d in ref_i[2:]:
        if d != "f":
            assert params[n].default == d, n
    assert list(inspect.signature(P.__init__).parameters) == ["self", "vae", "text_encoder", "tokenizer", "unet", "scheduler", "safety_checker",
                                                              "feature_extractor", "requires_safety_checker"]
    assert list(inspect.signature(P.from_pretrained).parameters) == ["save_dir", "kwargs"]
    # the reference defines the classes inside the function modules: those import paths resolve too
    from paint_with_words.paint_with_words import PaintWithWord_StableDiffusionPipeline as P2
    from paint_with_words.paint_with_words_inpaint import PaintWithWord_StableDiffusionInpaintPipeline as PI2
    assert P2 is P and PI2 is PI


_SIG_GLOBAL_K = 2.0


def _sig_helper(x):
    return 2.0 * x


def test_weight_function_signature_survives_fresh_lambdas():
    """The cache key of the per-step FALL-BACK graphs (pww_hip/sampler.py; the regular hipGraph path re-evaluates the weight
    function on the host every step and needs no key): the reference's callers build a fresh lambda per request (runner.py:104,
    gradio_pww.py:43) -- same code and constants must give the same key, a changed constant (in the code, in a NESTED code
    object, a closure cell, a default or a numeric global) a different one, and anything that cannot be proven constant (a
    helper function, a mutable object in a closure, a callable object) never matches: re-capture instead of a stale replay."""
    from pww_hip.sampler import weight_function_signature as sig

    def make(c):
        return lambda w, sigma, qk: c * w * math.log(1 + sigma) * qk.max()

    def make_lit():
        return lambda w, sigma, qk: 0.4 * w * math.log(1 + sigma) * qk.max()

    assert make(0.4) is not make(0.4) and sig(make(0.4)) == sig(make(0.4))
    assert sig(make(0.4)) != sig(make(0.5))
    assert sig(make_lit()) == sig(make_lit())
    assert sig(make_lit()) != sig(lambda w, sigma, qk: 0.5 * w * math.log(1 + sigma) * qk.max())
    assert sig(make_lit()) != sig(lambda w, sigma, qk: 0.4 * w * math.log(1 + sigma) * qk.std())
    f1 = lambda w, sigma, qk, k=2.0: k * w * qk.max()   # noqa: E731
    f2 = lambda w, sigma, qk, k=3.0: k * w * qk.max()   # noqa: E731
    assert sig(f1) != sig(f2)
    assert sig(cases.weight_fn_runner) == sig(cases.weight_fn_runner) != sig(cases.weight_fn_std)
    t = torch.ones(2)
    assert sig(lambda w, s, qk: t * w) != sig(lambda w, s, qk: t * w)       # a captured tensor / list / config object may have been mutated
    cfg = {"k": 0.4}
    fc = lambda w, s, qk: cfg["k"] * w * qk.max()   # noqa: E731
    assert sig(fc) != sig(fc)
    # constants inside nested code objects (inner lambdas / comprehensions) are part of the key
    n1 = lambda w, s, qk: (lambda: 0.4)() * w * qk.max()   # noqa: E731
    n1b = lambda w, s, qk: (lambda: 0.4)() * w * qk.max()   # noqa: E731
    n2 = lambda w, s, qk: (lambda: 0.5)() * w * qk.max()   # noqa: E731
    assert sig(n1) == sig(n1b) != sig(n2)
    # numeric globals are keyed by value, helper functions make the key unmatchable
    g1 = lambda w, s, qk: _SIG_GLOBAL_K * w * qk.max()   # noqa: E731
    assert sig(g1) == sig(lambda w, s, qk: _SIG_GLOBAL_K * w * qk.max())
    assert sig(lambda w, s, qk: _sig_helper(w) * qk.max()) != sig(lambda w, s, qk: _sig_helper(w) * qk.max())

    class Callable_:
        def __call__(self, w, s, qk):
            return 0.4 * w
    c = Callable_()
    assert sig(c) != sig(c)


def test_coeff_slots_reevaluate_the_weight_function_on_the_host():
    """hipGraph mode keeps the weight function's per-step Python scalar in device words (attention.CoeffSlots): the host
    re-evaluates the function on symbolic stand-ins each step. Checked here without a GPU: the symbolic evaluation returns the
    same scalar / statistic the real call forms, follows changed constants, and reports functions it cannot decompose."""
    from pww_hip.attention import ScaledW, _ProbeProxy, _symbolic_scalar, _NotSymbolic
    from pww_hip import ops
    w = torch.rand(16, 77)
    probe = lambda: _ProbeProxy((8, 16, 77), torch.float16, "cpu")   # noqa: E731
    sigma = torch.tensor(7.84)
    kind, scalar = _symbolic_scalar(cases.weight_fn_runner(ScaledW(w), sigma, probe()))
    assert kind == ops.STAT_MAX and abs(scalar - 0.4 * math.log(1 + 7.84)) < 1e-6
    kind, scalar = _symbolic_scalar(cases.weight_fn_std(ScaledW(w), sigma, probe()))
    assert kind == ops.STAT_STD and abs(scalar - 0.4 * math.log(1 + 7.84 ** 2)) < 1e-5
    kind, scalar = _symbolic_scalar((lambda w, s, qk: 0.25 * w)(ScaledW(w), sigma, probe()))
    assert kind == ops.STAT_NONE and scalar == 0.25
    assert _symbolic_scalar((lambda w, s, qk: 0.0)(ScaledW(w), sigma, probe())) is None
    assert _symbolic_scalar((lambda w, s, qk: torch.log(s + 1) * w)(ScaledW(w), sigma, probe())) is None              # tensor coefficient
    with pytest.raises(_NotSymbolic):
        (lambda w, s, qk: torch.log(s + 1) * w * qk.max())(ScaledW(w), sigma, probe())   # tensor coefficient times the statistic: needs its value
    with pytest.raises(_NotSymbolic):
        (lambda w, s, qk: w * qk.max() + qk.mean().sqrt())(ScaledW(w), sigma, probe())    # needs the statistic's value
    with pytest.raises(_NotSymbolic):
        (lambda w, s, qk: w * qk[0, 0, 0])(ScaledW(w), sigma, probe())                    # needs the scores themselves


def test_fold_context_per_image_maps():
    """Folding a batch whose images have their OWN contexts (paint_with_words_batch): rows [cond..., uncond...], weight
    maps stacked to [2n, 1, N, 77] with zero maps for the gated-out unconditional rows; a shared context stays [N, 77]."""
    from pww_hip.sampler import _fold_context
    from pww_hip.attention import ROW_GATE
    def ctx(seed):
        g = torch.Generator().manual_seed(seed)
        return {"CONTEXT_TENSOR": torch.randn(1, 77, 8, generator=g), "CROSS_ATTENTION_WEIGHT_16": torch.rand(16, 77, generator=g),
                "CROSS_ATTENTION_WEIGHT_ORIG": torch.rand(8, 8, 77, generator=g)}
    conds = [ctx(1), ctx(2), ctx(3)]
    unc = {"CONTEXT_TENSOR": torch.zeros(1, 77, 8), "CROSS_ATTENTION_WEIGHT_16": 0, "CROSS_ATTENTION_WEIGHT_ORIG": 0}
    f = _fold_context(conds, unc, 3, "cpu")
    assert f["CONTEXT_TENSOR"].shape == (6, 77, 8) and torch.equal(f["CONTEXT_TENSOR"][1], conds[1]["CONTEXT_TENSOR"][0])
    assert f["CROSS_ATTENTION_WEIGHT_16"].shape == (6, 1, 16, 77)
    assert torch.equal(f["CROSS_ATTENTION_WEIGHT_16"][2, 0], conds[2]["CROSS_ATTENTION_WEIGHT_16"]) and float(f["CROSS_ATTENTION_WEIGHT_16"][3:].abs().sum()) == 0.0
    assert f["CROSS_ATTENTION_WEIGHT_ORIG"].shape == (6, 8, 8, 77)
    assert f[ROW_GATE].tolist() == [1, 1, 1, 0, 0, 0]
    from pww_hip.attention import GATED_ROWS
    assert f[GATED_ROWS] == 3                 # what the gate holds, as a host-side int: the fused launch's work-distribution hint
    shared = _fold_context(conds[0], unc, 3, "cpu")
    assert shared["CROSS_ATTENTION_WEIGHT_16"] is conds[0]["CROSS_ATTENTION_WEIGHT_16"] and shared["CONTEXT_TENSOR"].shape == (6, 77, 8)
    with pytest.raises(ValueError):
        _fold_context(conds[:2], unc, 3, "cpu")


@pytest.mark.parametrize("gpus", [2, 8])
def test_bench_spawns_its_own_ranks_dry_run(gpus, tmp_path):
    """`python bench.py --gpus N --config 3` outside a launcher re-executes itself as N ranks (torch.distributed.run,
    127.0.0.1 rendezvous); on a box without GPUs `--dry-run` carries the run through rendezvous (gloo), the bucketed weight
    broadcast of a 1/8-width model and the request broadcast, and prints the contract line with value null -- with 2 ranks and
    with the 8 ranks of the driver's scaling run (one MIOpen user db per local rank)."""
    import subprocess
    import sys
    env = dict(os.environ, PWW_BENCH_VERBOSE="0", PWW_MIOPEN_DB_BASE=str(tmp_path / "miopen"))
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("MIOPEN_USER_DB_PATH", None)
    out = subprocess.run([sys.executable, os.path.join(cases.REPO, "bench.py"), "--gpus", str(gpus), "--config", "3", "--dry-run"],
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == gpus and rec["value"] is None and rec["dry_run"] is True and rec["scaling"] == "weak"
    assert rec["config"]["weight_broadcast"]["broadcast_bytes"] > 0 and rec["config"]["images_per_step"] == 8 * gpus
    assert rec["config"]["weight_broadcast_s"] is not None and rec["config"]["request_broadcast_s"] is not None
    assert sorted(os.listdir(tmp_path / "miopen")) == ["pww_rank%d" % r for r in range(gpus)]
    if gpus != 2:
        return
    assert "8 vertical stripes" in rec["config"]["workload"] and rec["config"]["baseline_config"] == 3
    # without --dry-run and without a GPU the run stops at the device check with a clear message
    out = subprocess.run([sys.executable, os.path.join(cases.REPO, "bench.py"), "--config", "4"], capture_output=True, text=True, timeout=600, env=env)
    if not torch.cuda.is_available():
        assert out.returncode != 0 and "needs a HIP device" in (out.stderr + out.stdout)


def test_bench_uneven_split_dry_run(tmp_path):
    """a global batch that does not divide by the rank count. `bench.py --dry-run --gpus 3 --global-batch 8`:
    three gloo ranks report -- each for itself, gathered -- 3 / 3 / 2 images and first seeds 0 / 3 / 6 (contiguous split, seeds by global
    index); stdout carries the ONE json line even though gloo prints its banners from C++ (fd 1 is redirected at the descriptor level)."""
    import subprocess
    import sys
    env = dict(os.environ, PWW_BENCH_VERBOSE="0", PWW_MIOPEN_DB_BASE=str(tmp_path / "miopen"))
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("MIOPEN_USER_DB_PATH", None)
    out = subprocess.run([sys.executable, os.path.join(cases.REPO, "bench.py"), "--gpus", "3", "--global-batch", "8", "--dry-run"],
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout)                       # nothing but the line
    assert rec["n_gpus"] == 3 and rec["config"]["images_per_step"] == 8
    assert rec["config"]["shards"] == [[0, 3], [3, 6], [6, 8]]
    assert rec["config"]["per_rank_images"] == [3, 3, 2] and rec["config"]["per_rank_first_seed"] == [0, 3, 6]


def test_adopt_miopen_db(tmp_path, monkeypatch):
    """bench.py --gpus N: rank 0 warms up first, the other ranks copy its MIOpen user db into their own directory before their first
    convolution (pww_hip.dist.adopt_miopen_db): files are copied, lock files are not, a user-chosen MIOPEN_USER_DB_PATH is left alone."""
    from pww_hip import dist as pdist
    base = tmp_path / "miopen"
    (base / "pww_rank0").mkdir(parents=True), (base / "pww_rank1").mkdir()
    (base / "pww_rank0" / "gfx950_256.HIP.ufdb.txt").write_text("record")
    (base / "pww_rank0" / "gfx950_256.HIP.udb.txt").write_text("perf")
    (base / "pww_rank0" / "gfx950_256.HIP.ufdb.txt.lock").write_text("")
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(base / "pww_rank1"))
    assert pdist.miopen_db_path(0) == str(base / "pww_rank0")
    assert pdist.adopt_miopen_db(0) == 2
    assert sorted(os.listdir(base / "pww_rank1")) == ["gfx950_256.HIP.udb.txt", "gfx950_256.HIP.ufdb.txt"]
    assert (base / "pww_rank1" / "gfx950_256.HIP.ufdb.txt").read_text() == "record"
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(base / "pww_rank0"))
    assert pdist.adopt_miopen_db(0) == 0                                   # the source rank itself
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(tmp_path / "users_own"))
    assert pdist.miopen_db_path(0) is None and pdist.adopt_miopen_db(0) == 0


def test_bench_parity_check_helper():
    """bench.py's `parity` object: the fixture itself passes with rel-L2 0, a perturbed latent fails above the bar,
    a run that is not the fixture's workload (other step count, --tiny) reports None, and only the images a rank holds are compared."""
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("pww_bench", os.path.join(cases.REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    args = argparse.Namespace(config=2, tiny=False, guidance=7.5)
    cfg = dict(bench.CONFIGS[2])
    g = np.load(os.path.join(cases.GOLDEN, "loop_sd15_example_plms30_oracle.npz"))
    lat = torch.from_numpy(g["latents"])
    par = bench.parity_check(args, cfg, lat, 0)
    assert par["ok"] and par["rel_l2"] == 0.0 and par["bar"] == 5e-2 and par["fixture"].endswith("loop_sd15_example_plms30_oracle.npz")
    bad = bench.parity_check(args, cfg, lat * 1.1, 0)
    assert not bad["ok"] and abs(bad["rel_l2"] - 0.1) < 1e-3
    assert bench.parity_check(args, dict(cfg, denoise_steps=4), lat, 0) is None
    assert bench.parity_check(argparse.Namespace(config=2, tiny=True, guidance=7.5), cfg, lat, 0) is None
    assert bench.parity_check(args, cfg, lat, 1) is None                     # this rank's shard starts behind the fixture's image
    # config 4: images 0 and 5 of the rank's eight (seeds 81, 86); fp16 config 3: the 1e-2 bar
    g4 = np.load(os.path.join(cases.GOLDEN, "loop_sd15_inpaint_lms30.npz"))
    lat4 = torch.zeros(8, 4, 64, 64)
    lat4[0], lat4[5] = torch.from_numpy(g4["latents_81"][0]), torch.from_numpy(g4["latents_86"][0])
    par4 = bench.parity_check(argparse.Namespace(config=4, tiny=False, guidance=7.5), dict(bench.CONFIGS[4]), lat4, 0)
    assert par4["ok"] and sorted(par4["per_image"]) == ["0", "5"]
    assert bench.PARITY_BARS == {"bf16": 5e-2, "fp16": 1e-2} and sorted(bench.PARITY_FIXTURES) == [2, 3, 4, 5]


def test_bench_workloads_build():
    """Every BASELINE workload of bench.py builds its request (arrays + color_context + prompt) and names its phrases."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pww_bench", os.path.join(cases.REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from sd_standin import HashTokenizer
    from pww_hip.conditioning import _parse_regions, _column_lists, _extract_seed_and_sigma_from_context
    tok = HashTokenizer()
    for cfg_id, n_regions, size in ((2, 5, 512), (3, 8, 512), (4, 4, 512), (5, 12, 768)):
        req = bench.make_request(cfg_id)
        assert req["rgb"].shape == (size, size, 3) and len(req["context"]) == n_regions
        ctx, seeds, _ = _extract_seed_and_sigma_from_context(dict(req["context"]))
        assert len(seeds) == (12 if cfg_id == 5 else 0)
        table = _parse_regions(ctx, tok)
        ids = tok([req["prompt"]], padding="max_length", max_length=77, truncation=True, return_tensors="pt")["input_ids"][0].tolist()
        cols = _column_lists(table, ids)
        assert sum(1 for c in cols if c) >= n_regions          # every region's phrase occurs in the prompt
        assert bench.CONFIGS[cfg_id]["wf"] in bench.weight_functions()
    assert bench.make_request(4)["mask"].shape == (512, 512) and bench.make_request(4)["init"].shape == (512, 512, 3)


def test_reference_runner_script_resolves_against_this_package(tmp_path):
    """The reference's OWN runner.py, unmodified (read from /root/reference, build box only), executed against this
    package: `from paint_with_words import paint_with_words, PaintWithWord_StableDiffusionPipeline` and its keyword call
    must resolve, pww_load_tools must run (stand-in diffusers / transformers / dotenv modules: tests/scripts/
    reference_env.py), and without a GPU the run must stop exactly where the modules move to "cuda:0" -- not at an
    ImportError / TypeError of the drop-in surface. The GPU box runs tests/scripts/runner_like.py to the saved image
    (tests/test_round2_gpu.py::test_runner_script_end_to_end)."""
    import subprocess
    import sys
    runner = "/root/reference/runner.py"
    if not os.path.isfile(runner):
        pytest.skip("reference checkout not present (GPU box)")
    os.symlink("/root/reference/contents", tmp_path / "contents")
    out = subprocess.run([sys.executable, os.path.join(cases.REPO, "tests", "scripts", "reference_env.py"), runner], cwd=tmp_path,
                         capture_output=True, text=True, timeout=600)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr[-3000:]
        return
    err = out.stderr
    assert out.returncode != 0
    assert "ImportError" not in err and "TypeError" not in err and "AttributeError" not in err, err[-3000:]
    assert "pww_load_tools" in err and "CompVis/stable-diffusion-v1-4" in out.stdout          # got as far as loading and placing the modules
    assert ("Torch not compiled with CUDA enabled" in err or "No HIP GPUs are available" in err or "HIP" in err.splitlines()[-1]
            or "CUDA" in err.splitlines()[-1]), err[-1500:]


def test_reference_runner_inpaint_script_resolves_against_this_package(tmp_path):
    """The reference's own runner_inpaint.py (:40-92), unmodified, like runner.py above: `from paint_with_words import
    paint_with_words_inpaint, PaintWithWord_StableDiffusionInpaintPipeline` and its keyword call must resolve against this
    package, pww_load_tools must run for "runwayml/stable-diffusion-inpainting" (stand-in modules with a 9-channel UNet), and
    without a GPU the run stops where the modules move to "cuda:0". The GPU box runs tests/scripts/runner_inpaint_like.py to
    the saved images (tests/test_round3_gpu.py::test_runner_inpaint_script_end_to_end)."""
    import subprocess
    import sys
    runner = "/root/reference/runner_inpaint.py"
    if not os.path.isfile(runner):
        pytest.skip("reference checkout not present (GPU box)")
    os.symlink("/root/reference/contents", tmp_path / "contents")
    out = subprocess.run([sys.executable, os.path.join(cases.REPO, "tests", "scripts", "reference_env.py"), runner], cwd=tmp_path,
                         capture_output=True, text=True, timeout=600)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stderr[-3000:]
        return
    err = out.stderr
    assert out.returncode != 0
    assert "ImportError" not in err and "TypeError" not in err and "AttributeError" not in err, err[-3000:]
    assert "pww_load_tools" in err and "runwayml/stable-diffusion-inpainting" in out.stdout
    assert ("Torch not compiled with CUDA enabled" in err or "No HIP GPUs are available" in err or "HIP" in err.splitlines()[-1]
            or "CUDA" in err.splitlines()[-1]), err[-1500:]


def test_pipeline_accepts_a_missing_color_map():
    """`pipe(prompt)` with the reference's defaults (color_map_image=None, color_context={}): its _image_context_seperator
    builds one dummy region over a 512 x 512 all-zero map (paint_with_words.py:239-243), i.e. plain Stable Diffusion. The
    conditioning builder must do the same instead of failing on `None`."""
    import sd_standin as S
    from pww_hip.conditioning import _encode_text_color_inputs
    text, tok = S.TinyTextEncoder(64, seed=1235), S.HashTokenizer()
    seeds, info, cond, uncond = _encode_text_color_inputs(text, tok, "cpu", None, {}, "a photo of a cat", "")
    assert seeds == {} and cond["CONTEXT_TENSOR"].shape == (1, 77, 64)
    assert cond["CROSS_ATTENTION_WEIGHT_4096"].shape == (4096, 77) and float(cond["CROSS_ATTENTION_WEIGHT_4096"].abs().sum()) == 0.0
    assert cond["CROSS_ATTENTION_WEIGHT_ORIG"].shape == (512, 512, 77) and uncond["CROSS_ATTENTION_WEIGHT_64"] == 0


@pytest.mark.slow
def test_kernel_invariants_static():
    """tools/check_kernel_invariants.py: compiler-dependent properties the measured kernel times rest on (register budgets, counted
    vmcnt waits of the Q ring, back-to-back LDS-direct copies), checked on the gfx950 ISA hipcc produces here. ~5 minutes of compiling:
    PWW_SLOW=1."""
    import subprocess
    import sys as _sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([_sys.executable, os.path.join(repo, "tools", "check_kernel_invariants.py")], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stdout[-3000:]


# ---- round 4 ------------------------------------------------------------------------------------------------------------------

def test_pww_context_builds_the_orig_map_on_first_access():
    """conditioning.PwWContext: the reference's dict protocol (:370-386) with CROSS_ATTENTION_WEIGHT_ORIG built when somebody
    indexes it (only inj_forward's KeyError path does, :95-101)."""
    from pww_hip.conditioning import PwWContext
    built = []
    ctx = PwWContext({"CONTEXT_TENSOR": 1, "CROSS_ATTENTION_WEIGHT_4096": 2}).set_lazy("CROSS_ATTENTION_WEIGHT_ORIG", lambda: built.append(1) or "MAP")
    assert "CROSS_ATTENTION_WEIGHT_ORIG" in ctx and ctx.pending("CROSS_ATTENTION_WEIGHT_ORIG") and not built
    assert "CROSS_ATTENTION_WEIGHT_ORIG" not in dict(ctx) and len(ctx) == 2
    with pytest.raises(KeyError):
        ctx["CROSS_ATTENTION_WEIGHT_1024"]                     # the reference's try / except KeyError still works (:92-95)
    twin = ctx.copy()
    assert isinstance(twin, PwWContext) and twin.pending("CROSS_ATTENTION_WEIGHT_ORIG")
    assert ctx["CROSS_ATTENTION_WEIGHT_ORIG"] == "MAP" and built == [1] and not ctx.pending("CROSS_ATTENTION_WEIGHT_ORIG")
    assert ctx["CROSS_ATTENTION_WEIGHT_ORIG"] == "MAP" and built == [1]          # built once
    assert dict(ctx)["CROSS_ATTENTION_WEIGHT_ORIG"] == "MAP"
    assert twin.get("CROSS_ATTENTION_WEIGHT_ORIG") == "MAP" and built == [1, 1]   # the copy made before builds its own
    assert twin.get("nope", 7) == 7
    ctx.update({"SIGMA": 3.0})
    assert ctx["SIGMA"] == 3.0


def test_weight_function_results_are_classified_for_graph_replay():
    """attention.CoeffSlots.classify: what a captured hipGraph holds per cross-attention call site -- a bias kernel with a
    statistic selector, or NO bias kernel -- so that a change of class between requests / steps forces a re-capture."""
    import math
    import torch
    from pww_hip.attention import CoeffSlots, ScaledW, _ProbeProxy
    from pww_hip import ops
    w = torch.zeros(16, 77)

    def run(f, sigma=5.0):
        return CoeffSlots.classify(f(ScaledW(w), sigma, _ProbeProxy((8, 16, 77), torch.float16, "cpu")))
    assert run(lambda w, s, qk: 0.4 * w * math.log(1 + s) * qk.max()) == (ops.STAT_MAX, pytest.approx(0.4 * math.log(6.0)))
    assert run(lambda w, s, qk: 0.4 * w * math.log(1 + s ** 2) * qk.std())[0] == ops.STAT_STD
    assert run(lambda w, s, qk: 0.1 * w)[0] == ops.STAT_NONE
    assert run(lambda w, s, qk: 0)[0] == CoeffSlots.NO_BIAS and run(lambda w, s, qk: 0.0)[0] == CoeffSlots.NO_BIAS
    assert run(lambda w, s, qk: torch.tensor(0.0))[0] == CoeffSlots.NO_BIAS
    assert run(lambda w, s, qk: 2.0 * qk.max())[0] == CoeffSlots.NO_BIAS         # a bare statistic: constant per row, cancels in softmax
    thresholded = lambda w, s, qk: 0.4 * w * qk.max() if s > 3 else 0               # noqa: E731
    assert run(thresholded, 5.0)[0] == ops.STAT_MAX and run(thresholded, 1.0)[0] == CoeffSlots.NO_BIAS
    assert run(lambda w, s, qk: w + 1.0) is None                                    # a tensor-valued bias: not representable by a device word


def test_block_plug_keeps_cpu_and_fp32_inputs_on_the_modules_own_forward():
    """pww_hip/blocks.py: the per-instance plug of ResnetBlock2D / GroupNorm (row a17) hands anything the HIP kernels do not take -- here CPU
    fp32 tensors, how the oracle runs the stand-in -- to the module's ORIGINAL forward, bit for bit, and uninstall() removes every trace."""
    import torch
    import torch.nn as nn
    from pww_hip import blocks
    from sd_standin import unet as U
    torch.manual_seed(0)
    res = U.ResnetBlock2D(32, 64, 128).eval().requires_grad_(False)
    norm = nn.GroupNorm(32, 64)
    holder = nn.ModuleList([res, norm])
    x, temb = torch.randn(2, 32, 8, 8), torch.randn(2, 128)
    with torch.no_grad():
        want, want_n = res(x, temb), norm(res(x, temb))
        assert blocks.install_blocks(holder) == (1, 1) and blocks.install_blocks(holder) == (1, 1)      # idempotent
        assert "forward" in res.__dict__ and "forward" in norm.__dict__ and "forward" not in res.norm1.__dict__
        assert torch.equal(res(x, temb), want) and torch.equal(norm(want), want_n)
        # the stock-op form of the fused helper (what a block falls back to for an input the kernels do not take) is the same arithmetic
        add = res.time_emb_proj(torch.nn.functional.silu(temb))
        h = res.conv1(torch.nn.functional.silu(res.norm1(x)))
        assert torch.equal(blocks.fused_group_norm(res.norm2, h, add=add, act="silu"), torch.nn.functional.silu(res.norm2(h + add[:, :, None, None])))
        blocks.uninstall_blocks(holder)
        assert "forward" not in res.__dict__ and "forward" not in norm.__dict__ and "_pww_orig_forward" not in res.__dict__
        assert torch.equal(res(x, temb), want)

    class Odd(nn.Module):               # a block named ResnetBlock2D that the restated forward does not cover keeps its own forward
        def __init__(self):
            super().__init__()
            self.norm1, self.norm2 = nn.GroupNorm(4, 8), nn.GroupNorm(4, 8)
            self.conv1 = self.conv2 = nn.Identity()
            self.time_embedding_norm = "scale_shift"
    Odd.__name__ = "ResnetBlock2D"
    odd = Odd()
    assert blocks.install_blocks(odd) == (0, 2) and "forward" not in odd.__dict__


def test_batched_time_embedding_projection_tracks_its_source_weights():
    """blocks.TembProjections: one GEMM for all blocks' time_emb_proj(silu(temb)); the concatenated copy follows in-place updates,
    replaced parameters and casts of the source weights; the result is cached on the temb tensor object only."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from pww_hip.blocks import TembProjections
    torch.manual_seed(1)
    lins = [nn.Linear(16, n) for n in (8, 20, 32)]            # (20: the next block still starts on a multiple of 8 columns)
    blocks_ = [type("B", (), {"time_emb_proj": lin})() for lin in lins]
    plan = TembProjections()
    slots = [plan.register(b) for b in blocks_]
    assert [s[1] for s in slots] == [0, 8, 32] and plan.width == 64
    temb = torch.randn(3, 16)
    with torch.no_grad():
        out = plan.project(temb)
        assert plan.project(temb) is out                       # cached on this tensor object ...
        assert plan.project(temb.clone()) is not out           # ... and nowhere else
        for lin, (_, off, n) in zip(lins, slots):
            assert torch.allclose(out[:, off:off + n], lin(F.silu(temb)), atol=1e-6)
        lins[1].weight.mul_(2.0)                               # in-place update: version counter moves
        assert torch.allclose(plan.project(temb.clone())[:, 8:28], lins[1](F.silu(temb)), atol=1e-6)
        lins[2].weight = nn.Parameter(torch.randn(32, 16))     # replaced parameter
        assert torch.allclose(plan.project(temb.clone())[:, 32:64], lins[2](F.silu(temb)), atol=1e-6)
        t64 = temb.double()
        for lin in lins:
            lin.double()
        assert torch.allclose(plan.project(t64)[:, 0:8], lins[0](F.silu(t64)), atol=1e-12)


def test_block_plug_is_safe_on_later_diffusers_signatures():
    """VERDICT round 4 item 4 / ADVICE: diffusers 0.21 - 0.26 call `resnet(hidden_states, temb, scale=...)`, `GEGLU(hidden_states, scale)`
    and `BasicTransformerBlock(hidden_states, attention_mask=..., encoder_hidden_states=..., timestep=...)`; 0.10.0's Transformer2DModel
    calls `block(hidden_states, context=..., timestep=None)`. The per-instance plug accepts the 0.10.0 call (a None timestep included) and
    hands anything beyond it to the module's OWN forward, arguments untouched -- never a TypeError. Fake modules carry the later signatures."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from pww_hip import blocks

    class ResnetBlock2D(nn.Module):                 # 0.21-style: forward(input_tensor, temb, scale=1.0)
        def __init__(self):
            super().__init__()
            self.norm1, self.norm2 = nn.GroupNorm(4, 8), nn.GroupNorm(4, 8)
            self.conv1, self.conv2 = nn.Conv2d(8, 8, 3, padding=1), nn.Conv2d(8, 8, 3, padding=1)
            self.time_emb_proj = nn.Linear(16, 8)
            self.nonlinearity = nn.SiLU()
            self.seen = None

        def forward(self, input_tensor, temb, scale=1.0):
            self.seen = scale
            h = self.conv1(F.silu(self.norm1(input_tensor)))
            h = h + self.time_emb_proj(F.silu(temb))[:, :, None, None] * scale
            return input_tensor + self.conv2(F.silu(self.norm2(h)))

    class GEGLU(nn.Module):                         # 0.21-style: forward(hidden_states, scale=1.0)
        def __init__(self):
            super().__init__()
            self.proj = nn.Linear(8, 32)
            self.seen = None

        def forward(self, hidden_states, scale=1.0):
            self.seen = scale
            a, g = (self.proj(hidden_states) * scale).chunk(2, dim=-1)
            return a * F.gelu(g)

    class BasicTransformerBlock(nn.Module):         # later signature: encoder_hidden_states=..., timestep=..., cross_attention_kwargs=...
        def __init__(self):
            super().__init__()
            self.norm1, self.norm2, self.norm3 = nn.LayerNorm(8), nn.LayerNorm(8), nn.LayerNorm(8)
            self.attn1 = self.attn2 = self.ff = nn.Identity()
            self.seen = None

        def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, timestep=None,
                    cross_attention_kwargs=None, class_labels=None, context=None):
            self.seen = dict(encoder_hidden_states=encoder_hidden_states, timestep=timestep, context=context, cross_attention_kwargs=cross_attention_kwargs)
            return self.norm1(hidden_states) + hidden_states

    torch.manual_seed(3)
    res, geglu, blk = ResnetBlock2D().eval(), GEGLU().eval(), BasicTransformerBlock().eval()
    model = nn.ModuleList([res, geglu, blk])
    x, temb, tok = torch.randn(2, 8, 4, 4), torch.randn(2, 16), torch.randn(2, 5, 8)
    with torch.no_grad():
        want_r, want_g, want_b = res(x, temb, scale=0.5), geglu(tok, 0.5), blk(tok, encoder_hidden_states="ctx", timestep=7)
        blocks.reset_stats()
        blocks.install_blocks(model)
        try:
            assert all("_pww_orig_forward" in m.__dict__ for m in (res, geglu, blk))
            res.seen = geglu.seen = blk.seen = None
            assert torch.equal(res(x, temb, scale=0.5), want_r) and res.seen == 0.5
            assert torch.equal(res(x, temb, 0.5), want_r)                                    # positional extra
            assert torch.equal(geglu(tok, 0.5), want_g) and geglu.seen == 0.5
            assert torch.equal(geglu(tok, scale=0.5), want_g)
            assert torch.equal(blk(tok, encoder_hidden_states="ctx", timestep=7), want_b)
            assert blk.seen["encoder_hidden_states"] == "ctx" and blk.seen["timestep"] == 7
            blk(tok, None, None, None, None, {"scale": 1.0})                                  # six positionals of the later signature
            assert blk.seen["cross_attention_kwargs"] == {"scale": 1.0}
            # the 0.10.0 call: context + a None timestep is the covered form (CPU tensors: handed to the module's own forward, not a TypeError)
            blk(tok, context="c", timestep=None)
            assert blk.seen["context"] == "c" and blk.seen["timestep"] is None
            st = blocks.stats()
            assert st["resnet_block"]["declined"] == 2 and st["geglu"]["declined"] == 2 and st["transformer_block"]["declined"] == 3
            assert st["hit_rate"] == 0.0
        finally:
            blocks.uninstall_blocks(model)
        blocks.reset_stats()
        assert blocks.stats()["hit_rate"] is None


def test_time_embedding_cache_follows_in_place_updates_of_temb():
    """a caller that keeps ONE temb tensor and updates it in place between forwards (static buffers, hipGraph-style input
    copies) must not get the previous step's projection: the cache entry on the tensor is keyed by its version counter and data pointer."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from pww_hip.blocks import TembProjections
    torch.manual_seed(2)
    lin = nn.Linear(16, 8)
    plan = TembProjections()
    plan.register(type("B", (), {"time_emb_proj": lin})())
    temb = torch.randn(2, 16)
    with torch.no_grad():
        a = plan.project(temb)
        assert plan.project(temb) is a
        temb.mul_(-1.5)                                                     # in place: same object, new values
        b = plan.project(temb)
        assert b is not a and torch.allclose(b[:, :8], lin(F.silu(temb)), atol=1e-6)
        temb.copy_(torch.randn(2, 16))                                      # a static input buffer refilled
        assert torch.allclose(plan.project(temb)[:, :8], lin(F.silu(temb)), atol=1e-6)
        view = temb[:]                                                      # another tensor object on the same storage: its own cache slot
        assert torch.allclose(plan.project(view)[:, :8], lin(F.silu(temb)), atol=1e-6)


def test_qproj_route_follows_the_measured_table(monkeypatch):
    """attention.qproj_route: `to_q` + statistic as one launch only where profiles/r04_qproj.md says the route wins."""
    import pww_hip.attention as A
    monkeypatch.setattr(A, "QPROJ_STAT", "1")
    assert A.qproj_route(320, 40) and A.qproj_route(320, 64) and A.qproj_route(640, 80)           # SD1.5 N = 4096 / SD2.1 N = 9216 / SD1.5 N = 1024
    assert not A.qproj_route(640, 64) and not A.qproj_route(1280, 160) and not A.qproj_route(1280, 64)
    monkeypatch.setattr(A, "QPROJ_STAT", "all")
    assert A.qproj_route(1280, 64)
    monkeypatch.setattr(A, "QPROJ_STAT", "0")
    assert not A.qproj_route(320, 40)


def test_fused_projection_entry_point_says_what_it_takes(experiments_lib):
    """pww_cross_attn_out_supported is host logic (no GPU): the shapes pww_cross_attn_fwd_parts_out takes -- H * D = 320 with D <= 64,
    64 <= M <= 128, dense bias rows shared by the heads, at most 64 non-zero map columns -- and nothing else; the Python op refuses CPU
    tensors like every other op. Since round 6 an EXPERIMENTS-library entry point (measured slower / a tie: no product switch selects it)."""
    import ctypes
    import pww_hip
    from pww_hip import _lib, ops, attention
    lib = _lib.load_experiments()

    def desc(H, D, N=4096, M=77, bias_stride=(0, 0, 77, 1), dtype=1):
        d = _lib.AttnDesc()
        d.dtype, d.B, d.H, d.N, d.M, d.D = dtype, 2, H, N, M, D
        d.q_stride[:] = [N * H * D, D, H * D]
        d.bias_stride[:] = list(bias_stride)
        return d
    ok = lambda d, C=320, cols=32: bool(lib.pww_cross_attn_out_supported(ctypes.byref(d), C, cols))      # noqa: E731
    assert ok(desc(8, 40)) and ok(desc(5, 64)) and ok(desc(10, 32)) and ok(desc(8, 40, dtype=0))
    assert ok(desc(8, 40, M=64), cols=0) and ok(desc(8, 40, M=128))
    assert not ok(desc(8, 80), C=640) and not ok(desc(8, 160), C=1280) and not ok(desc(4, 80))           # other widths, D > 64
    assert not ok(desc(8, 40), C=640)                                                                     # C must be H * D
    assert not ok(desc(8, 40, M=40)) and not ok(desc(8, 40, M=129))
    assert not ok(desc(8, 40), cols=0)                                                                    # 77 keys without a column bound: 80 > 64 columns
    assert not ok(desc(8, 40, bias_stride=(0, 4096 * 77, 77, 1))) and not ok(desc(8, 40, bias_stride=(0, 0, 1, 4096)))      # a map per head / transposed rows
    assert not lib.pww_cross_attn_out_supported(None, 320, 32)
    x = torch.randn(1, 128, 320).half()
    with pytest.raises(pww_hip.PwwHipError):
        ops.attention_out(x, x[:, :77], x[:, :77], 8, 1.0, torch.rand(128, 77), torch.randn(320, 320).half())
    assert attention.FUSE_TO_OUT is False and not hasattr(_lib.load(), "pww_cross_attn_fwd_parts_out") or _lib.has_experiments()


def test_attention_route_table():
    """ops._attention_route: which launch ops.attention takes, from which arguments are given and the key count alone -- every row of the
    table in DESIGN.md section 5, the tie-break of the statistic-free long context over the partials / in-launch rows included."""
    from pww_hip import ops
    route = ops._attention_route
    stats, parts, scratch = object(), object(), object()          # stand-ins: the decision looks at `is None` only
    kinds = (ops.STAT_NONE, ops.STAT_MAX, ops.STAT_STD)
    for M in (77, 128, 129, 4096):
        for sc in (None, scratch):
            for pt in (None, parts):
                for stat in [None] + [(s, kind, 0.5) for s in (None, stats) for kind in kinds]:
                    assert route(False, stat, sc, pt, M) == "self"                   # no bias: whatever else is given
                assert route(True, None, sc, pt, M) == "plain"
                for kind in kinds:
                    assert route(True, (stats, kind, 0.5), sc, pt, M) == "stat"      # the statistics come with the call
    # stat = (None, STAT_NONE, scalar) over more keys than one K/V stage, no partials: the launch without a key limit, scratch or not
    assert ops.FUSED_MAX_KEYS == 128
    assert route(True, (None, ops.STAT_NONE, 0.5), None, None, 129) == "stat"
    assert route(True, (None, ops.STAT_NONE, 0.5), scratch, None, 129) == "stat"
    # ... and not at 128 keys, not with partials, not with a statistic to form
    assert route(True, (None, ops.STAT_NONE, 0.5), None, None, 128) == "parts"
    assert route(True, (None, ops.STAT_NONE, 0.5), scratch, None, 128) == "fused"
    assert route(True, (None, ops.STAT_NONE, 0.5), None, parts, 129) == "parts"
    assert route(True, (None, ops.STAT_NONE, 0.5), scratch, parts, 129) == "fused"
    for M in (77, 128, 129):
        for pt in (None, parts):
            assert route(True, (None, ops.STAT_MAX, 0.5), None, pt, M) == "parts"
            assert route(True, (None, ops.STAT_MAX, 0.5), scratch, pt, M) == "fused"


def test_stale_library_fails_with_the_rebuild_hint(monkeypatch, tmp_path):
    """A libpww_hip.so older than the package (here: ABI 1.25, and none of the symbols added since) ends in PwwHipError with the build
    command -- not in the AttributeError of the first symbol it lacks."""
    import pww_hip._lib as L

    class Stale:
        def __init__(self, path):
            self.pww_version = lambda: 125
            self.pww_last_error = lambda: b""
    so = tmp_path / "libpww_hip.so"
    so.write_bytes(b"")
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(so))
    monkeypatch.setattr(L.ctypes, "CDLL", Stale)
    with pytest.raises(L.PwwHipError, match=r"1\.25 .*rebuild: python paint-with-words-sd_amd/build\.py"):
        L.load()
    assert L._lib is None
