"""LoRA adapters without a device: the two key grammars and the stacks they give, the limits, the keywords of the entry points, the row
plan, the stock-torch formula against merged weights, libpww_hip_lora.so's header / exports / argument checks, and the merged-UNet oracle
loop against its recorded fixture."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import lora_cases as L
import pww_cases as cases
import region_prompt_cases as R
from gpu_util import rel_l2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKY, GROUND = (90, 206, 255), (74, 18, 1)


@pytest.fixture()
def unet():
    return cases.build_tools("tiny")[1]


def _stacks(unet):
    from pww_hip import lora
    st = lora.state_of(unet)
    out = {}
    for path, layer in st.layers.items():
        groups = [("to_q", "to_k", "to_v"), ("to_out.0",)] if path.endswith("attn1") else [("to_q",), ("to_k", "to_v"), ("to_out.0",)]
        for g in groups:
            out[(path, g)] = layer.stack(g)
    return out


# ---- loading
def test_both_grammars_give_the_same_stacks_and_alpha_scales_b(unet):
    from pww_hip import lora
    f = L.make_factors(unet, seed=3, rank=4, alpha=None)
    lora.load_lora(unet, L.kohya_dict(f), "k")
    k = _stacks(unet)
    lora.unload_lora(unet, "k")
    lora.load_lora(unet, L.peft_dict(f), "p")
    p = _stacks(unet)
    lora.unload_lora(unet, "p")
    lora.load_lora(unet, L.peft_dict(f, prefix=""), "q")
    q = _stacks(unet)
    assert k.keys() == p.keys() == q.keys() and len(k) == 5 * len(L.attention_paths(unet)) // 2
    for key in k:
        for a, b, c in zip(k[key], p[key], q[key]):
            assert torch.equal(a, b) and torch.equal(a, c)
    # rank 4 is padded to 32 with exact zeros; the stacks' layout; values are the factors' (alpha defaults to the rank: factor 1)
    path = L.attention_paths(unet)[0]
    A, B = k[(path, ("to_q", "to_k", "to_v"))]
    C = f[(path, "to_q")][0].shape[1]
    assert tuple(A.shape) == (1, 3, 32, C) and tuple(B.shape) == (1, 3, C, 32) and A.dtype == B.dtype == torch.float32
    assert not A[:, :, 4:].any() and not B[..., 4:].any()
    for g, t in enumerate(("to_q", "to_k", "to_v")):
        assert torch.equal(A[0, g, :4], f[(path, t)][0]) and torch.equal(B[0, g, :, :4], f[(path, t)][1])
    # an explicit alpha: B carries alpha / rank, in both grammars alike
    lora.unload_lora(unet, "q")
    f2 = {key: (d, u, 2.0) for key, (d, u, _) in f.items()}
    lora.load_lora(unet, L.kohya_dict(f2), "k2")
    k2 = _stacks(unet)
    lora.unload_lora(unet, "k2")
    lora.load_lora(unet, L.peft_dict(f2), "p2")
    p2 = _stacks(unet)
    for key in k:
        assert torch.equal(k2[key][0], k[key][0]) and torch.equal(k2[key][1], k[key][1] * 0.5) and torch.equal(p2[key][1], k2[key][1])


def test_two_adapters_share_one_padded_rank_and_a_partial_adapter_is_zero_elsewhere(unet):
    from pww_hip import lora
    lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=1, rank=4, targets=("to_q",))), "small")
    lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=2, rank=40)), "big")
    st = lora.state_of(unet)
    assert lora.loras(unet) == ["small", "big"] and st.rank_pad == 64 and st.index("big") == 1
    for (path, g), (A, B) in _stacks(unet).items():
        assert A.shape[0] == B.shape[0] == 2 and A.shape[2] == B.shape[3] == 64 and A.shape[1] == len(g)
        assert not A[1, :, 40:].any() and not A[0, :, 4:].any()
        for s, t in enumerate(g):
            assert bool(A[0, s].any()) == (t == "to_q") and bool(B[0, s].any()) == (t == "to_q")


def test_foreign_keys_shapes_and_limits(unet):
    from pww_hip import lora
    f = L.make_factors(unet, seed=5, rank=4)
    good = L.kohya_dict(f)
    foreign = {"lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": torch.zeros(4, 8),
               "lora_unet_mid_block_attentions_0_proj_in.lora_up.weight": torch.zeros(8, 4),
               "unet.mid_block.attentions.0.transformer_blocks.0.ff.net.2.lora_A.weight": torch.zeros(4, 8)}
    with pytest.raises(ValueError) as e:
        lora.load_lora(unet, dict(good, **foreign), "x")
    assert all(k in str(e.value) for k in foreign) and lora.loras(unet) == []
    ad = lora.load_lora(unet, dict(good, **foreign), "x", strict=False)
    assert sorted(ad.ignored) == sorted(foreign) and ad.rank == 4 and len(ad.factors) == len(f)
    with pytest.raises(ValueError, match="already loaded"):
        lora.load_lora(unet, good, "x")
    # a factor that does not fit the UNet always raises
    key = next(k for k in good if k.endswith("lora_down.weight"))
    for strict in (True, False):
        with pytest.raises(ValueError, match="factors"):
            lora.load_lora(unet, dict(good, **{key: torch.zeros(4, 7)}), "bad", strict=strict)
    with pytest.raises(ValueError, match="rank 129"):
        lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=6, rank=129, targets=("to_q",))), "wide")
    lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=6, rank=128, targets=("to_q",))), "r128")
    assert lora.state_of(unet).rank_pad == 128
    for i in range(6):
        lora.load_lora(unet, good, "n%d" % i)
    assert len(lora.loras(unet)) == 8
    with pytest.raises(ValueError, match="at most 8"):
        lora.load_lora(unet, good, "ninth")
    with pytest.raises(ValueError, match="not loaded"):
        lora.unload_lora(unet, "ninth")


def test_unload_restores_the_adapter_free_state_and_base_weights_are_never_touched(unet):
    from pww_hip import lora
    before = {k: v.clone() for k, v in unet.state_dict().items()}
    attrs = {p: set(m.__dict__) for p, m in unet.named_modules()}
    lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=1)), "a")
    lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=2)), "b")
    touched = [p for p, m in unet.named_modules() if "_pww_lora" in m.__dict__]
    assert touched == L.attention_paths(unet)
    g1 = lora.state_of(unet).signature()
    lora.unload_lora(unet, "a")
    g2 = lora.state_of(unet).signature()
    assert lora.loras(unet) == ["b"] and g1 != g2 and g1[:2] == g2[:2] == ("lora", 32)
    lora.unload_lora(unet, "b")
    assert lora.loras(unet) == [] and lora.state_of(unet) is None
    assert {p: set(m.__dict__) for p, m in unet.named_modules()} == attrs
    after = unet.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)


def test_safetensors_round_trip(unet, tmp_path):
    from safetensors.torch import save_file
    from pww_hip import lora
    f = L.make_factors(unet, seed=9, rank=8, alpha=4.0)
    path = tmp_path / "adapter.safetensors"
    save_file(L.kohya_dict(f), str(path))
    lora.load_lora(unet, path, "file")
    a = _stacks(unet)
    lora.unload_lora(unet, "file")
    lora.load_lora(unet, L.kohya_dict(f), "dict")
    b = _stacks(unet)
    assert all(torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) for k in a)


# ---- the keywords
def _entry_points():
    pw = importlib.import_module("paint_with_words.paint_with_words")
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    return [pw.paint_with_words, pw.paint_with_words_batch, inp.paint_with_words_inpaint, inp.paint_with_words_inpaint_batch]


TWO = {SKY: "stormy sky", GROUND: "wet street"}
BAD = [(dict(lora="missing"), "not loaded"),
       (dict(lora=("a", float("inf"))), "finite"),
       (dict(lora=("a", float("nan"))), "finite"),
       (dict(lora=("a", True)), "finite"),
       (dict(lora=3), "name or"),
       (dict(lora=("a", 1.0, 2.0)), "name or"),
       (dict(region_prompts=TWO, region_loras={SKY: "missing"}), "not loaded"),
       (dict(region_prompts=TWO, region_loras={SKY: ("a", float("-inf"))}), "finite"),
       (dict(region_prompts=TWO, region_loras={(1, 2, 3): "a"}), "not a key of the request's region_prompts"),
       (dict(region_loras={SKY: "a"}), "not a key of the request's region_prompts"),
       (dict(region_prompts=TWO, region_loras={SKY: "a", "#5aceff": "a"}), "twice"),
       (dict(region_prompts=TWO, region_loras="a"), "must be a dict"),
       (dict(region_prompts=TWO, region_loras=[{SKY: "a"}]), "batch form|entries for")]


@pytest.mark.parametrize("kw,match", BAD, ids=["%s%d" % (m[:8], i) for i, (_, m) in enumerate(BAD)])
def test_bad_keywords_raise_before_a_model_is_touched(unet, kw, match):
    """The tools hold nothing but a UNet with the adapter "a": everything else is None, so a ValueError means the check came first."""
    from pww_hip import lora
    lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=1, targets=("to_q",))), "a")
    tools = (None, unet, None, None, None)
    eps = _entry_points()
    for f, args in ((eps[0], ()), (eps[1], ({}, None, "", [0, 1])), (eps[2], ()), (eps[3], ({}, None, None, None, "", [0, 1]))):
        with pytest.raises(ValueError, match=match):
            f(*args, preloaded_utils=tools, **kw)
    pipes = importlib.import_module("paint_with_words.pipelines")
    for cls in (pipes.PaintWithWord_StableDiffusionPipeline, pipes.PaintWithWord_StableDiffusionInpaintPipeline):
        assert cls.lora is None and cls.region_loras is None
        pipe = cls.__new__(cls)
        pipe.unet = unet
        for k, v in kw.items():
            setattr(pipe, k, v)
        with pytest.raises(ValueError, match=match):
            pipe("a prompt", **({"image": 0, "mask_image": 0} if "Inpaint" in cls.__name__ else {}))


def test_keywords_without_tools_and_the_batch_length(unet):
    from pww_hip import conditioning as C, lora
    eps = _entry_points()
    with pytest.raises(ValueError, match="not loaded"):
        eps[0](lora="a")          # no preloaded_utils: nothing can be loaded on a UNet this call would create
    lora.load_lora(unet, L.kohya_dict(L.make_factors(unet, seed=1, targets=("to_q",))), "a")
    tools = (None, unet, None, None, None)
    for f, args in ((eps[1], ({}, None, "")), (eps[3], ({}, None, None, None, ""))):
        with pytest.raises(ValueError, match="2 entries for 3 requests"):
            f(*args, [0, 1, 2], preloaded_utils=tools, region_prompts=TWO, region_loras=[{SKY: "a"}, None])
    assert C.check_loras(None, None) is None and C.check_loras(None, {}, TWO, tools=tools) is None
    assert C.check_loras("a", None, tools=tools) == (("a", 1.0), [None])
    got = C.check_loras(("a", 0.5), [{"#5aceff": "a"}, None], [TWO, TWO], n_requests=2, tools=tools)
    assert got == (("a", 0.5), [{SKY: ("a", 1.0)}, None])
    for f in eps:
        names = list(__import__("inspect").signature(f).parameters)
        assert names.index("lora") > names.index("strength") and names[names.index("lora") + 1] == "region_loras"


# ---- the row plan
def test_row_plan_equals_the_hand_written_rows():
    """n = 2 images, K = 2 regions, the second region with its own adapter, a global one with scale 0.5: rows [base x 2, region 1 x 2,
    region 2 x 2, unconditional x 2]; the eager calls take their one row from the same plan."""
    from pww_hip import lora
    index = {"g": 0, "own": 1}.__getitem__
    colors = [[SKY, GROUND], [SKY, GROUND]]
    adapters, scales = lora.row_plan(2, colors, ("g", 0.5), [{GROUND: ("own", 2.0)}, {GROUND: ("own", 2.0)}], index)
    assert adapters == [0, 0, 0, 0, 1, 1, 0, 0] and scales == [0.5, 0.5, 0.5, 0.5, 2.0, 2.0, 0.5, 0.5]
    # per-image dicts: image 1 has none of its own
    adapters, scales = lora.row_plan(2, colors, ("g", 0.5), [{GROUND: ("own", 2.0)}, None], index)
    assert adapters == [0, 0, 0, 0, 1, 0, 0, 0] and scales == [0.5, 0.5, 0.5, 0.5, 2.0, 0.5, 0.5, 0.5]
    # no global adapter: -1 wherever no region entry applies
    adapters, scales = lora.row_plan(2, colors, None, [{SKY: ("own", 1.0)}, {SKY: ("g", -1.0)}], index)
    assert adapters == [-1, -1, 1, 0, -1, -1, -1, -1] and scales == [0.0, 0.0, 1.0, -1.0, 0.0, 0.0, 0.0, 0.0]
    # without regions: [cond x n, uncond x n]
    assert lora.row_plan(2, [[], []], ("own", 0.25), None, index) == ([1, 1, 1, 1], [0.25] * 4)
    assert lora.row_plan(1, [[]], None, None, index) == ([-1, -1], [0.0, 0.0])


class _Recorder(torch.nn.Module):
    """A UNet stand-in that records the assignment in force at each call."""

    def __init__(self, state_of):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls, self.in_channels, self._state_of = [], 4, state_of

    def forward(self, x, t, encoder_hidden_states=None):
        st = self._state_of(self)
        self.calls.append((x.shape[0], st.row_adapter[:x.shape[0]].tolist(), st.row_scale[:x.shape[0]].tolist()))
        from types import SimpleNamespace
        return SimpleNamespace(sample=torch.zeros_like(x[:, :4]))


@pytest.mark.parametrize("mode", ["eager", "folded"])
def test_the_sampler_writes_the_plan_for_folded_and_for_the_unfolded_calls(mode):
    """The same plan through PwWSampler on the CPU (fp32: the blend is the torch one): folded, one call sees all eight rows; eager, the
    cond / region / uncond calls of each image see their own row."""
    from pww_hip import lora, sampler as S
    from sd_standin import LMSDiscreteScheduler
    unet = _Recorder(lora.state_of)
    st = lora.state_of(unet, create=True)
    st.adapters = [lora.LoraAdapter("g", {("x", "to_q"): (torch.zeros(4, 8), torch.zeros(8, 4), 4.0)}, ()),
                   lora.LoraAdapter("own", {("x", "to_q"): (torch.zeros(4, 8), torch.zeros(8, 4), 4.0)}, ())]
    sch = LMSDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    sch.set_timesteps(1)
    n, K = 2, 2
    ctx = lambda: {"CONTEXT_TENSOR": torch.zeros(1, 77, 8), "CROSS_ATTENTION_WEIGHT_64": 0}      # noqa: E731
    plan = {"contexts": [ctx() for _ in range(K)], "masks": torch.zeros(K, 8, 8), "weights": torch.ones(K), "scales": torch.ones(K)}
    rows = lora.row_plan(n, [[SKY, GROUND]] * n, ("g", 0.5), [{GROUND: ("own", 2.0)}, None], st.index)
    smp = S.PwWSampler(unet, sch, mode)
    smp.sample(ctx(), ctx(), torch.zeros(n, 4, 8, 8), sch.timesteps, 7.5, lambda w, s, qk: 0.0, regions=plan, lora_rows=rows)
    if mode == "folded":
        assert unet.calls == [(8, [0, 0, 0, 0, 1, 0, 0, 0], [0.5, 0.5, 0.5, 0.5, 2.0, 0.5, 0.5, 0.5])]
    else:       # per image: cond, region 1, region 2, uncond
        assert unet.calls == [(1, [0], [0.5]), (1, [0], [0.5]), (1, [1], [2.0]), (1, [0], [0.5]),
                              (1, [0], [0.5]), (1, [0], [0.5]), (1, [0], [0.5]), (1, [0], [0.5])]
    # a request without the keywords on a UNet with adapters: every row is -1
    unet.calls.clear()
    smp.sample(ctx(), ctx(), torch.zeros(n, 4, 8, 8), sch.timesteps, 7.5, lambda w, s, qk: 0.0)
    assert all(a == [-1] * b and s == [0.0] * b for b, a, s in unet.calls)
    with pytest.raises(ValueError, match="rows"):
        smp.sample(ctx(), ctx(), torch.zeros(n, 4, 8, 8), sch.timesteps, 7.5, lambda w, s, qk: 0.0, lora_rows=([0], [1.0]))


# ---- the formula
def test_torch_formula_in_fp64_equals_merged_weights():
    """x (W + s B A)^T per row, three rows with adapters [-1, 0, 1], two segments with their own factors."""
    from pww_hip import ops
    g = torch.Generator().manual_seed(0)
    Rr, T, K, N, n, seg, r = 3, 5, 8, 12, 2, 2, 4
    x, W = torch.randn(Rr, T, K, generator=g, dtype=torch.float64), torch.randn(N, K, generator=g, dtype=torch.float64)
    A, B = torch.randn(n, seg, r, K, generator=g, dtype=torch.float64), torch.randn(n, seg, N // seg, r, generator=g, dtype=torch.float64)
    ra, rs = torch.tensor([-1, 0, 1], dtype=torch.int32), torch.tensor([1.0, 0.5, -2.0])
    base = x @ W.t()
    y = ops.lora_update_torch(base.clone(), x, A, B, ra, rs, seg)
    assert torch.equal(y[0], base[0])
    for i in (1, 2):
        BA = torch.cat([B[ra[i], s] @ A[ra[i], s] for s in range(seg)], dim=0)
        ref = x[i] @ (W + float(rs[i]) * BA).t()
        assert (y[i] - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    # scale 0 keeps the row's bits
    y0 = ops.lora_update_torch(base.clone(), x, A, B, torch.tensor([0, 1, 0], dtype=torch.int32), torch.zeros(3), seg)
    assert torch.equal(y0, base)


# ---- the library
@pytest.fixture(scope="module")
def lib(built_lib):
    sys.path.insert(0, os.path.join(REPO, "paint-with-words-sd_amd"))
    import build as pww_build
    pww_build.build_lora()
    from pww_hip import _lib
    return _lib.load_lora()


def test_header_exports_and_the_loader_tables(lib):
    import build as pww_build
    import pww_hip
    from pww_hip import _lib
    header = open(os.path.join(REPO, "include", "pww_hip_lora.h")).read()
    declared = set(re.findall(r"\b(pww_lora_\w+)\s*\(", header))
    assert declared == set(_lib.LORA_EXPORTS), declared ^ set(_lib.LORA_EXPORTS)
    assert all(hasattr(lib, n) for n in _lib.LORA_EXPORTS) and lib.pww_lora_version() == 100 == _lib.LORA_MIN_VERSION
    assert set(_lib.LORA_EXPORTS).isdisjoint(pww_hip.EXPORTS)
    assert ctypes.sizeof(_lib.LoraDesc) == 72
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LORA_LIB_PATH], capture_output=True, text=True).stdout
    vis = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {v for v in vis if v.startswith("pww_")} == set(_lib.LORA_EXPORTS)
    # a sibling table of the loader, not a fifth key of SIDE; the build table has it, and build() walks that table
    assert "lora" not in _lib.SIDE and tuple(_lib.SIDE_MORE) == ("lora",) and _lib.side_spec("lora") is _lib.SIDE_MORE["lora"]
    assert _lib.side_spec("linear") is _lib.SIDE["linear"] and _lib.load_side("lora") is lib and _lib.load_lora() is lib
    spec = _lib.SIDE_MORE["lora"]
    assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_lora_version", "pww_lora_last_error"} and not spec["missing_ok"]
    assert tuple(pww_build.SIDE_LIBS) == tuple(_lib.SIDE) + tuple(_lib.SIDE_MORE)
    assert pww_build.SIDE_LIBS["lora"][0] == "pww_lora.hip" and "-fvisibility=hidden" in pww_build.LORA_UNITS[0][1]
    assert pww_build.LIB_LORA == _lib.LORA_LIB_PATH
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "for name in pww_build.SIDE_LIBS" in entry and "zip(pww_build.SIDE_LIBS" not in entry


def _desc(R=4, T=77, K=320, N=960, n_seg=3, rank=32, n_adapters=2, dtype=1, strides=None):
    from pww_hip import _lib
    xr, xt, yr, yt = strides or (T * K, K, T * N, N)
    return _lib.LoraDesc(ctypes.sizeof(_lib.LoraDesc), dtype, R, T, K, N, n_seg, rank, n_adapters, 0, xr, xt, yr, yt)


def test_bad_descriptors_return_the_documented_code_and_launch_nothing(lib):
    """No device here: a launch would fail with PWW_EHIP, so EINVAL / ENOTSUP means the check ran in front of the HIP runtime."""
    from pww_hip import _lib
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    names = ("x", "a", "b", "row_adapter", "row_scale", "y")

    def call(d, **ptr):
        args = [ptr.get(n, p) for n in names]
        return lib.pww_lora_fwd(*args[:6], ctypes.byref(d) if d is not None else None, None)
    short = _desc()
    short.size = 16
    table = [(short, {}, _lib.PWW_EINVAL, b"older")] + [(_desc(), {n: None}, _lib.PWW_EINVAL, b"required") for n in names] + [
        (None, {}, _lib.PWW_EINVAL, b"missing"),
        (_desc(n_seg=4, N=1280), {}, _lib.PWW_EINVAL, b"segments"), (_desc(n_seg=0), {}, _lib.PWW_EINVAL, b"segments"),
        (_desc(n_adapters=0), {}, _lib.PWW_EINVAL, b"adapters"), (_desc(n_adapters=9), {}, _lib.PWW_EINVAL, b"adapters"),
        (_desc(R=0), {}, _lib.PWW_EINVAL, b"sizes"), (_desc(T=0), {}, _lib.PWW_EINVAL, b"sizes"),
        (_desc(rank=48), {}, _lib.PWW_ENOTSUP, b"rank"), (_desc(rank=0), {}, _lib.PWW_ENOTSUP, b"rank"), (_desc(rank=160), {}, _lib.PWW_ENOTSUP, b"rank"),
        (_desc(K=40), {}, _lib.PWW_ENOTSUP, b"multiple of 32"), (_desc(N=968), {}, _lib.PWW_ENOTSUP, b"multiple of 16"),
        (_desc(N=72, n_seg=3), {}, _lib.PWW_ENOTSUP, b"multiple of 16"), (_desc(dtype=2), {}, _lib.PWW_ENOTSUP, b"dtype"),
        (_desc(strides=(77 * 324, 324, 77 * 960, 960)), {}, _lib.PWW_ENOTSUP, b"strides"),
        (_desc(strides=(77 * 320, 320, 77 * 960, 952)), {}, _lib.PWW_ENOTSUP, b"strides"),
        (_desc(strides=(76 * 320, 320, 77 * 960, 960)), {}, _lib.PWW_ENOTSUP, b"strides"),
        (_desc(), {"y": p + 8}, _lib.PWW_ENOTSUP, b"aligned"), (_desc(), {"a": p + 2}, _lib.PWW_ENOTSUP, b"aligned"),
        (_desc(R=4096, T=4096, K=320, N=320, n_seg=1), {}, _lib.PWW_ENOTSUP, b"2^31"),
    ]
    for d, ptr, code, text in table:
        rc = call(d, **ptr)
        err = lib.pww_lora_last_error()
        assert rc == code and err and text in err, (rc, code, err, ptr)


def test_ops_declines_what_the_library_would_refuse():
    from pww_hip import ops
    x, y = torch.zeros(2, 5, 32), torch.zeros(2, 5, 16)
    A, B = torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 16, 32)
    assert not ops.lora_takes(y, x, A, B, 1)                                    # not on a device, not a half type


# ---- the oracle loop and its fixture
def test_recorded_oracle_reproduces_and_the_adapters_are_visible():
    """Re-runs the global-adapter loop (and its adapter-free twin) and holds the fixture to them; the recorded latents keep the adapters
    10 x the loop caps apart: with against without, and the two regions' adapters swapped. Measured here (fp32 CPU):
    global / without 1.300, regions / regions_without 2.145, swapped / regions 1.293 (1.302 the other way round)."""
    rec = L.recorded()
    for name in ("global", "without"):
        again = L.oracle_loop(**L.RECORDED[name])
        assert rel_l2(again, rec[name]) <= R.GOLDEN_TOL, name
    assert rel_l2(rec["without"], R.recorded()["without"]) <= R.GOLDEN_TOL      # no adapter, no regions: the region-prompt fixture's loop
    cap = max(L.CAP.values())
    assert rel_l2(rec["global"], rec["without"]) >= 10 * cap
    assert rel_l2(rec["regions"], rec["regions_without"]) >= 10 * cap
    assert rel_l2(rec["swapped"], rec["regions"]) >= 10 * cap and rel_l2(rec["regions"], rec["swapped"]) >= 10 * cap


@pytest.mark.slow
@pytest.mark.parametrize("name", ["regions_without", "regions", "swapped"])
def test_recorded_region_loops_reproduce(name):
    assert rel_l2(L.oracle_loop(**L.RECORDED[name]), L.recorded()[name]) <= R.GOLDEN_TOL
