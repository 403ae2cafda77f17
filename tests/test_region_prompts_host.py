"""Region prompts, host side (no GPU): the `region_prompts` / `region_base_weight` / `region_feather` keywords, their checks, the plan
conditioning builds, the folded context with K more row classes, libpww_hip_regions.so's export list and argument checks, and the loop's host
layers against the oracle loop of tests/region_prompt_cases.py.

The launches themselves are pinned on the device (tests/test_region_prompts_gpu.py); here `ops.region_masks` is the numpy restatement of
tests/region_prompt_cases.py and the attention launches are torch restatements, as in tests/test_negative_regions_host.py."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pww_cases as cases
import region_prompt_cases as R
from host_standins import cpu_masks  # noqa: F401  (fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = 64
KEYS = (64, 16, 4, 1)
WEIGHT_KEYS = ["CROSS_ATTENTION_WEIGHT_%d" % k for k in KEYS]
POS_CONTEXT = {(0, 0, 0): "cat,1.0", (255, 255, 255): "dog,1.5"}
POS_PROMPT = "a photo of a cat and a dog"
GREEN, WHITE, BLACK = (13, 255, 0), (255, 255, 255), (0, 0, 0)
TWO = {GREEN: "an old oak tree, autumn", WHITE: ("a white dog", 0.5, 3.0)}


def _color_map():
    img = np.zeros((SIDE, SIDE, 3), dtype=np.uint8)                 # left half black, right half white, a green square in the middle
    img[:, SIDE // 2:] = 255
    img[24:40, 24:40] = GREEN
    return img


def _tools():
    from sd_standin import HashTokenizer, TinyTextEncoder
    return TinyTextEncoder(32, seed=1235), HashTokenizer()


@pytest.fixture
def cpu_regions(monkeypatch, cpu_masks):
    from pww_hip import ops
    monkeypatch.setattr(ops, "region_masks", R.cpu_region_masks)


def _encode(pos=None, prompt=POS_PROMPT, uncond_prompt="", **kw):
    from pww_hip.conditioning import _encode_text_color_inputs
    text, tok = _tools()
    return _encode_text_color_inputs(text, tok, "cpu", _color_map(), dict(POS_CONTEXT) if pos is None else pos, prompt, uncond_prompt, **kw)


def _plan(regions, uncond, guidance=7.5, **kw):
    from pww_hip.conditioning import encode_region_prompts
    text, tok = _tools()
    return encode_region_prompts(text, tok, "cpu", _color_map(), regions, guidance, uncond, **kw)


def _entry_points():
    pw = importlib.import_module("paint_with_words.paint_with_words")
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    return [pw.paint_with_words, pw.paint_with_words_batch, inp.paint_with_words_inpaint, inp.paint_with_words_inpaint_batch]


def test_keywords_on_the_four_entry_points_and_the_pipeline_attributes():
    for f in _entry_points():
        params = inspect.signature(f).parameters
        names = list(params)
        assert params["region_prompts"].default is None and params["region_base_weight"].default == 0.0 and params["region_feather"].default == 0.0
        at = names.index("region_prompts")
        assert names[at:at + 3] == ["region_prompts", "region_base_weight", "region_feather"], f.__qualname__
        assert at > names.index("strength") and names[-1] == "max_prompt_chunks" and names[at + 3] == "max_prompt_chunks"
    pipes = importlib.import_module("paint_with_words.pipelines")
    for cls in (pipes.PaintWithWord_StableDiffusionPipeline, pipes.PaintWithWord_StableDiffusionInpaintPipeline):
        assert cls.region_prompts is None and cls.region_base_weight == 0.0 and cls.region_feather == 0.0
        assert not {"region_prompts", "region_base_weight", "region_feather"} & set(inspect.signature(cls.__call__).parameters)


BAD = [(dict(region_prompts={GREEN: "a tree"}, region_base_weight=1.0), "region_base_weight"),
       (dict(region_prompts={GREEN: "a tree"}, region_base_weight=-0.1), "region_base_weight"),
       (dict(region_base_weight=float("nan")), "region_base_weight"),
       (dict(region_feather=8.5), "region_feather"),
       (dict(region_feather=-1.0), "region_feather"),
       (dict(region_feather=True), "region_feather"),
       (dict(region_prompts="a tree"), "must be a dict"),
       (dict(region_prompts={(i, 0, 0): "p%d" % i for i in range(9)}), "1 to 8 regions"),
       (dict(region_prompts={(256, 0, 0): "a tree"}), "colour"),
       (dict(region_prompts={"#12345": "a tree"}), "colour"),
       (dict(region_prompts={GREEN: "a tree", "#0dff00": "another tree"}), "twice"),
       (dict(region_prompts={GREEN: ("a tree", 0.0)}), "weight"),
       (dict(region_prompts={GREEN: ("a tree", 1.5)}), "weight"),
       (dict(region_prompts={GREEN: ("a tree", 1.0, float("inf"))}), "guidance_scale"),
       (dict(region_prompts={GREEN: ("a tree", 1.0, 7.5, 1)}), "prompt or"),
       (dict(region_prompts={GREEN: 3}), "prompt or"),
       (dict(region_prompts={GREEN: "a tree"}, negative_color_context={WHITE: "dog,1.0"}), "negative_color_context")]


@pytest.mark.parametrize("kw,match", BAD, ids=[m + str(i) for i, (_, m) in enumerate(BAD)])
def test_bad_values_raise_before_the_tools_are_touched(kw, match):
    """No tools are given and none can be loaded here: a ValueError means the check ran in front of everything else."""
    eps = _entry_points()
    for f, args in ((eps[0], ()), (eps[1], ({}, None, "", [0])), (eps[2], ()), (eps[3], ({}, None, None, None, "", [0]))):
        with pytest.raises(ValueError, match=match):
            f(*args, **kw)
    pipes = importlib.import_module("paint_with_words.pipelines")
    for cls in (pipes.PaintWithWord_StableDiffusionPipeline, pipes.PaintWithWord_StableDiffusionInpaintPipeline):
        pipe = cls.__new__(cls)
        for k, v in kw.items():
            setattr(pipe, k, v)
        with pytest.raises(ValueError, match=match):
            pipe("a prompt", **({"image": 0, "mask_image": 0} if "Inpaint" in cls.__name__ else {}))


def test_batch_forms_and_the_grammar():
    from pww_hip import conditioning as C
    eps = _entry_points()
    one, two = {GREEN: "a tree"}, dict(TWO)
    for f, args in ((eps[1], ({}, None, "")), (eps[3], ({}, None, None, None, ""))):
        with pytest.raises(ValueError, match="same number of regions"):
            f(*args, [0, 1], region_prompts=[one, two])
        with pytest.raises(ValueError, match="same number of regions"):
            f(*args, [0, 1], region_prompts=[one, None])
        with pytest.raises(ValueError, match="2 entries for 3 requests"):
            f(*args, [0, 1, 2], region_prompts=[one, one])
        with pytest.raises(ValueError, match="negative_color_context"):
            f(*args, [0, 1], region_prompts=one, negative_color_context=[None, {WHITE: "dog,1.0"}])
    with pytest.raises(ValueError, match="batch form"):
        C.check_region_prompts([one])
    assert C.check_region_prompts(None) == 0 and C.check_region_prompts({}) == 0 and C.check_region_prompts([None, {}], n_requests=2) == 0
    assert C.check_region_prompts(two) == 2 and C.check_region_prompts([two, dict(two)], n_requests=2) == 2
    assert C.check_region_prompts(one, negative_color_context={}) == 1 and C.check_region_prompts(None, negative_color_context={WHITE: "dog,1.0"}) == 0
    assert C.check_region_prompts(one, 0.999, 8.0) == 1
    # prompts may contain commas; colours as tuples, lists of ints or "#rrggbb"; weight and scale default to 1 and the call's
    got = C.region_entries({GREEN: "a tree, a bush, moss", "#ffffff": ("a dog", 0.25), (0, 0, 0): ["a cat", 1, None], (1, 2, 3): ("x", 0.5, 2)})
    assert got == [(GREEN, "a tree, a bush, moss", 1.0, None), (WHITE, "a dog", 0.25, None), (BLACK, "a cat", 1.0, None), ((1, 2, 3), "x", 0.5, 2.0)]
    pw = importlib.import_module("paint_with_words.paint_with_words")
    assert pw._region_requests(None, 2) is None and pw._region_requests({}, 3) is None and pw._region_requests([None, {}], 2) is None
    assert pw._region_requests(one, 2) == [one, one] and pw._region_requests([one, two], 2) == [one, two]


def test_plan_of_one_request(cpu_regions):
    """The region dicts are built like the unconditional dict (integer 0 in every slot, the oracle's builder with the region prompt as its
    unconditional prompt), masks are the box means, weights carry (1 - beta) in fp32, scales default to the call's."""
    from oracle import pww_oracle as O
    text, tok = _tools()
    _, _, cond, uncond = _encode()
    plan = _plan(dict(TWO), uncond, guidance=6.0, region_base_weight=0.3)
    assert sorted(plan) == ["contexts", "masks", "scales", "weights"] and len(plan["contexts"]) == 2
    for ctx, prompt in zip(plan["contexts"], ("an old oak tree, autumn", "a white dog")):
        want = O.encode_text_color_inputs(text, tok, _color_map(), dict(POS_CONTEXT), POS_PROMPT, prompt)[3]
        assert type(ctx) is dict and sorted(ctx) == sorted(want) == sorted(uncond)
        assert all(ctx[k] == 0 and isinstance(ctx[k], int) for k in ctx if k != "CONTEXT_TENSOR")
        torch.testing.assert_close(ctx["CONTEXT_TENSOR"], want["CONTEXT_TENSOR"])
    m = plan["masks"]
    assert m.dtype == torch.float32 and tuple(m.shape) == (2, 8, 8)
    assert float(m[0, 3:5, 3:5].min()) == 1.0 and float(m[0].sum()) == 4.0             # the 16 x 16 square: 2 x 2 latent pixels
    assert float(m[1, :, 4:].sum()) == 32.0 - 2.0 and float(m[1, :, :4].sum()) == 0.0      # the white half less the square's share
    keep = np.float32(1.0) - np.float32(0.3)
    assert plan["weights"].dtype == torch.float32 and plan["weights"].tolist() == [float(keep * np.float32(1.0)), float(keep * np.float32(0.5))]
    assert plan["scales"].tolist() == [6.0, 3.0]
    # feathered: still at most 1 in sum, the square's mass spreads out and is kept (the normalisation by the taps inside the plane)
    f = _plan(dict(TWO), uncond, region_feather=1.5)["masks"]
    assert float(f.sum(0).max()) <= 1.0 + 1e-6 and 0.0 < float(f[0, 2, 2]) < float(f[0, 3, 3]) < 1.0
    # a request without a colour map cannot carry region prompts
    from pww_hip.conditioning import encode_region_prompts
    with pytest.raises(ValueError, match="color map"):
        encode_region_prompts(text, tok, "cpu", None, dict(TWO), 7.5, uncond)


def test_fold_regions_rows_gate_padding_and_chunks(cpu_regions):
    from pww_hip.sampler import _fold_regions, _fold_context
    from pww_hip.attention import ROW_GATE, GATED_ROWS, COND_ROWS, BIAS_COLS
    from pww_hip.conditioning import PwWContext
    _, _, cond, uncond = _encode()
    plan = _plan(dict(TWO), uncond)
    n, K = 2, 2
    f = _fold_regions(cond, plan, uncond, n, "cpu")
    base = _fold_context(cond, uncond, n, "cpu")
    assert isinstance(f, PwWContext) and list(f) == list(base) and COND_ROWS not in f
    assert f[ROW_GATE].tolist() == [1.0, 1.0] + [0.0] * 6 and f[ROW_GATE].dtype == torch.float32 and f[GATED_ROWS] == n and f[BIAS_COLS] == base[BIAS_COLS]
    ct = f["CONTEXT_TENSOR"]
    assert tuple(ct.shape) == ((K + 2) * n, 77, 32) and ct.is_contiguous()
    rows = [cond] * 2 + [plan["contexts"][0]] * 2 + [plan["contexts"][1]] * 2 + [uncond] * 2
    for b, d in enumerate(rows):
        assert torch.equal(ct[b], d["CONTEXT_TENSOR"][0]), b
    for k, key in zip(KEYS, WEIGHT_KEYS):                      # shared maps stay [N, 77]
        assert f[key] is cond[key] and tuple(f[key].shape) == (k, 77)
    assert f.pending("CROSS_ATTENTION_WEIGHT_ORIG")
    # per-image conditioning and per-image plans: the stacked maps are zero for every row past n, the rows of image i are request i's
    _, _, cond_b, uncond_b = _encode(pos={(0, 0, 0): "dog,0.7"})
    plan_b = _plan({WHITE: "a sleeping cat", BLACK: ("night sky", 1.0, 2.0)}, uncond_b)
    g = _fold_regions([cond, cond_b], [plan, plan_b], [uncond, uncond_b], n, "cpu")
    assert g[ROW_GATE].tolist() == [1.0, 1.0] + [0.0] * 6 and g[GATED_ROWS] == n
    for k, key in zip(KEYS, WEIGHT_KEYS):
        assert tuple(g[key].shape) == ((K + 2) * n, 1, k, 77) and float(g[key][n:].abs().sum()) == 0.0
        assert torch.equal(g[key][0, 0], cond[key]) and torch.equal(g[key][1, 0], cond_b[key])
    assert torch.equal(g["CONTEXT_TENSOR"][3], plan_b["contexts"][0]["CONTEXT_TENSOR"][0]) and torch.equal(g["CONTEXT_TENSOR"][4], plan["contexts"][1]["CONTEXT_TENSOR"][0])
    assert torch.equal(g["CONTEXT_TENSOR"][7], uncond_b["CONTEXT_TENSOR"][0])
    orig = g["CROSS_ATTENTION_WEIGHT_ORIG"]                     # built on first access, padded like the maps
    assert tuple(orig.shape) == ((K + 2) * n, SIDE, SIDE, 77) and float(orig[n:].abs().sum()) == 0.0 and torch.equal(orig[1], cond_b["CROSS_ATTENTION_WEIGHT_ORIG"])
    # the hipGraph signature (tensor shapes and ints): other prompts, masks and scales at the same K share it; K and on / off do not
    shape_sig = lambda d: sorted((k, tuple(v.shape)) for k, v in d.items() if torch.is_tensor(v) and not k.endswith("_ORIG"))      # noqa: E731
    int_sig = lambda d: sorted((k, v) for k, v in d.items() if isinstance(v, int))                    # noqa: E731
    f2 = _fold_regions(cond, _plan({BLACK: ("x", 0.3, 1.0), GREEN: "y"}, uncond, region_feather=2.0), uncond, n, "cpu")
    assert shape_sig(f2) == shape_sig(f) and int_sig(f2) == int_sig(f) and not torch.equal(f2["CONTEXT_TENSOR"], f["CONTEXT_TENSOR"])
    f1 = _fold_regions(cond, _plan({GREEN: "y"}, uncond), uncond, n, "cpu")
    assert shape_sig(f1) != shape_sig(f) and shape_sig(base) != shape_sig(f) and shape_sig(base) != shape_sig(f1)
    # a batch whose images differ in K cannot be stacked; negative regions are refused
    with pytest.raises(ValueError, match="same number of regions"):
        _fold_regions([cond, cond_b], [plan, _plan({GREEN: "y"}, uncond_b)], [uncond, uncond_b], n, "cpu")
    _, _, cond_n, uncond_n = _encode(uncond_prompt="a tree", negative_color_context={GREEN: "a tree,1.0"})
    with pytest.raises(ValueError, match="negative regions"):
        _fold_regions(cond_n, plan, uncond_n, n, "cpu")


def test_region_prompts_count_in_the_chunks_of_a_call(cpu_regions):
    from pww_hip.sampler import _fold_regions
    pw = importlib.import_module("paint_with_words.paint_with_words")
    text, tok = _tools()
    words = lambda k, stem="word": " ".join("%s%d" % (stem, i) for i in range(k))      # noqa: E731
    regions = {GREEN: words(100, "leaf"), WHITE: "a dog"}
    texts = [e[1] for e in pw.region_entries(regions)]
    assert pw._batch_prompt_chunks(tok, [POS_PROMPT, ""] + texts, 3) == 2 and pw._batch_prompt_chunks(tok, [POS_PROMPT, ""] + texts, 1) == 1
    _, _, cond, uncond = _encode(max_prompt_chunks=3, min_prompt_chunks=2)
    assert tuple(cond["CONTEXT_TENSOR"].shape) == (1, 154, 32) and tuple(uncond["CONTEXT_TENSOR"].shape) == (1, 154, 32)
    plan = _plan(regions, uncond)
    assert [tuple(c["CONTEXT_TENSOR"].shape) for c in plan["contexts"]] == [(1, 154, 32)] * 2
    f = _fold_regions(cond, plan, uncond, 1, "cpu")
    assert tuple(f["CONTEXT_TENSOR"].shape) == (4, 154, 32) and tuple(f["CROSS_ATTENTION_WEIGHT_64"].shape) == (64, 154)
    # the long prompt's second chunk is what chunk_prompt makes of it: 75 tokens, then the other 25
    from pww_hip.conditioning import chunk_prompt
    _, rows = chunk_prompt(tok, regions[GREEN], 2, 2)
    want = torch.cat([text(torch.tensor([r]))[0] for r in rows], dim=1)
    torch.testing.assert_close(plan["contexts"][0]["CONTEXT_TENSOR"], want)
    # under the default cap everything is cut at 77 and a mismatch cannot arise
    _, _, cond1, uncond1 = _encode()
    assert tuple(_plan(regions, uncond1)["contexts"][0]["CONTEXT_TENSOR"].shape) == (1, 77, 32)


def test_fp32_blend_of_the_sampler_is_the_restatement_bit_for_bit():
    """What an fp32 UNet's rows are combined with (sampler.region_blend_fp32) against the numpy restatement of the launch."""
    from pww_hip.sampler import region_blend_fp32
    g = torch.Generator().manual_seed(3)
    for n, K, hw in ((1, 1, (5, 7)), (3, 3, (8, 8)), (2, 8, (4, 6))):
        eps = torch.randn((K + 2) * n, 4, *hw, generator=g)
        masks = torch.rand(n, K, *hw, generator=g) / K
        weights, scales = torch.rand(n, K, generator=g), torch.rand(n, K, generator=g) * 10
        got = region_blend_fp32(eps, masks, weights, scales, 7.5)
        assert np.array_equal(got.numpy(), R.blend(eps.numpy(), masks.numpy(), weights.numpy(), scales.numpy(), 7.5)), (n, K)
    # K = 1 with an all-zero mask is classifier-free guidance
    eps = torch.randn(3, 4, 5, 7, generator=g)
    got = region_blend_fp32(eps, torch.zeros(1, 1, 5, 7), torch.ones(1, 1), torch.full((1, 1), 3.0), 7.5)
    assert torch.equal(got, eps[2:] + 7.5 * (eps[:1] - eps[2:]))


# ---- libpww_hip_regions.so without a device ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built_lib):
    sys.path.insert(0, os.path.join(REPO, "paint-with-words-sd_amd"))
    import build as pww_build
    pww_build.build_regions()
    from pww_hip import _lib
    return _lib.load_regions()


def test_header_and_exports(lib):
    from pww_hip import _lib, conditioning as C
    import pww_hip
    header = open(os.path.join(REPO, "include", "pww_hip_regions.h")).read()
    declared = set(re.findall(r"\b(pww_regions_\w+)\s*\(", header))
    assert declared == set(_lib.REGIONS_EXPORTS), declared ^ set(_lib.REGIONS_EXPORTS)
    assert all(hasattr(lib, n) for n in _lib.REGIONS_EXPORTS) and lib.pww_regions_version() == 100
    assert set(_lib.REGIONS_EXPORTS).isdisjoint(pww_hip.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.REGIONS_LIB_PATH], capture_output=True, text=True).stdout
    vis = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {v for v in vis if v.startswith("pww_")} == set(_lib.REGIONS_EXPORTS)
    # the header's bounds are the package's
    consts = {k: float(v.rstrip("f")) for k, v in re.findall(r"#define (PWW_REGIONS_MAX\w*) ([0-9.]+f?)", header)}
    assert consts == {"PWW_REGIONS_MAX": _lib.REGIONS_MAX, "PWW_REGIONS_MAX_PLANE": _lib.REGIONS_MAX_PLANE, "PWW_REGIONS_MAX_FEATHER": _lib.REGIONS_MAX_FEATHER}
    assert C.MAX_REGION_PROMPTS == _lib.REGIONS_MAX and C.MAX_REGION_FEATHER == _lib.REGIONS_MAX_FEATHER
    # the product library is what it was: its own export list and version do not know the feature
    assert not [n for n in pww_hip.EXPORTS if "region" in n]
    sys.path.insert(0, os.path.join(REPO, "paint-with-words-sd_amd"))
    import build as pww_build
    assert pww_build.PER_FILE_FLAGS["pww_regions.hip"] == ["-ffp-contract=off"] and "-fvisibility=hidden" in pww_build.REGIONS_UNITS[0][1]


def test_argument_checks_run_before_any_hip_call(lib):
    from pww_hip import _lib
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    colors = (ctypes.c_uint8 * 24)()
    err = lib.pww_regions_last_error
    masks = lambda rgb=p, H=512, W=512, c=colors, K=5, s=0.0, out=p: lib.pww_regions_masks(rgb, H, W, c, K, s, out, None)       # noqa: E731
    assert masks(rgb=None) == _lib.PWW_EINVAL and b"required" in err()
    assert masks(c=None) == _lib.PWW_EINVAL and masks(out=None) == _lib.PWW_EINVAL
    assert masks(K=0) == _lib.PWW_EINVAL and masks(K=9) == _lib.PWW_EINVAL and b"regions" in err()
    assert masks(H=7) == _lib.PWW_EINVAL and masks(W=0) == _lib.PWW_EINVAL and b"8 x 8" in err()
    assert masks(s=-0.5) == _lib.PWW_EINVAL and masks(s=8.5) == _lib.PWW_EINVAL and masks(s=float("nan")) == _lib.PWW_EINVAL and b"feather" in err()
    assert masks(H=776, W=768) == _lib.PWW_ENOTSUP and b"plane" in err()                # 97 x 96 latent pixels
    combine = lambda eps=p, m=p, w=p, s=p, out=p, n=1, K=5, C=4, hw=4096, dt=0: lib.pww_regions_combine(eps, m, w, s, 7.5, out, n, K, C, hw, dt, None)  # noqa: E731
    for name in ("eps", "m", "w", "s", "out"):
        assert combine(**{name: None}) == _lib.PWW_EINVAL and b"required" in err(), name
    assert combine(K=0) == _lib.PWW_EINVAL and combine(K=9) == _lib.PWW_EINVAL
    assert combine(n=0) == _lib.PWW_EINVAL and combine(n=65536) == _lib.PWW_EINVAL and combine(C=0) == _lib.PWW_EINVAL and combine(hw=0) == _lib.PWW_EINVAL
    assert combine(dt=2) == _lib.PWW_ENOTSUP and b"dtype" in err()
    assert combine(hw=1 << 31) == _lib.PWW_ENOTSUP and combine(n=65535, C=4096, hw=1 << 20) == _lib.PWW_ENOTSUP and b"2^40" in err()


def test_wrappers_refuse_what_the_launches_cannot_take():
    from pww_hip import ops
    from pww_hip._lib import PwwHipError
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.region_masks(torch.zeros(64, 64, 3, dtype=torch.uint8), [GREEN])
    with pytest.raises(PwwHipError, match="HIP device"):
        ops.region_combine(torch.zeros(3, 4, 8, 8, dtype=torch.float16), torch.zeros(1, 1, 8, 8), torch.ones(1, 1), torch.ones(1, 1), 7.5)


# ---- the loop's host layers against the oracle loop, on the CPU ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_loops():
    return {(steps, on): R.oracle_loop(R.REGIONS if on else None, steps=steps) for steps, on in ((3, True), (3, False), (10, True), (10, False))}


def test_fixture_is_visible_in_the_oracle(oracle_loops):
    """The fixture moves the oracle's final latent by far more than twice the widest cap the HIP path is held to (bf16: 1e-1);
    profiles/region_prompts.md records 0.379. The three regions measured there cover 0.043, 0.091 and 0.489 of the plane."""
    from gpu_util import rel_l2
    d = rel_l2(oracle_loops[(10, True)], oracle_loops[(10, False)])
    print("oracle: rel-L2(with region prompts, without) = %.3e" % d)
    assert d >= 2 * R.CAP[torch.bfloat16]
    assert abs(d - R.ORACLE_VISIBLE) <= 0.1 * R.ORACLE_VISIBLE
    m = R.region_masks(cases.load_example_rgb(), list(R.REGIONS))
    assert [round(float(v), 3) for v in m[:3].mean(axis=(1, 2))] == [0.043, 0.091, 0.489] and float(m[:3].sum(0).max()) == 1.0
    assert float(m.sum(0).max()) <= 1.0
    # the record the GPU tests compare against is this loop
    rec = R.recorded()
    assert set(rec) == set(R.RECORDED)
    for name, on in (("with", True), ("without", False)):
        assert rel_l2(rec[name], oracle_loops[(10, on)]) <= R.GOLDEN_TOL, name


@pytest.mark.slow
def test_fixture_variants_in_the_oracle(oracle_loops):
    """Rotated prompts, the 15 / 2 scales and beta = 0.5 against the fixture, and the fixture at qk_gain 2 (guidance 7.5 and 12)."""
    from gpu_util import rel_l2
    base = oracle_loops[(10, True)]
    want = {"rotated": (dict(regions=R.rotated()), 0.213), "scales": (dict(regions=R.with_scales(R.ALT_SCALES)), 0.213), "beta": (dict(regions=R.REGIONS, beta=0.5), 0.200)}
    rec = R.recorded()
    for name, (kw, figure) in want.items():
        lat = R.oracle_loop(**kw)
        d = rel_l2(lat, base)
        print("oracle: %s vs the fixture: rel-L2 %.3e" % (name, d))
        assert abs(d - figure) <= 0.1 * figure, name
        assert kw == {"regions": R.RECORDED[name]["regions"], **({"beta": 0.5} if name == "beta" else {})} and rel_l2(rec[name], lat) <= R.GOLDEN_TOL, name
    for guidance, figure in ((7.5, 0.209), (12.0, 0.314)):
        d = rel_l2(R.oracle_loop(R.REGIONS, qk_gain=2.0, guidance=guidance), R.oracle_loop(None, qk_gain=2.0, guidance=guidance))
        print("oracle: qk_gain 2, guidance %g, with vs without: rel-L2 %.3e" % (guidance, d))
        assert abs(d - figure) <= 0.1 * figure, guidance


def _host_loop(monkeypatch, mode, steps=3, **kw):
    from PIL import Image
    import paint_with_words as pw
    from gpu_util import install_unfused, uninstall_all
    from pww_hip import ops, sampler as S
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")

    def install_folded(unet):
        for m in unet.modules():
            if m.__class__.__name__ == "CrossAttention":
                m.__class__.__call__ = R.folded_forward

    class NoWatch:      # (the hand-off error words live on the device)
        def poll(self, wait=False):
            pass

        def post(self, modules):
            return False

    monkeypatch.setattr(pww_mod, "DEFAULT_MODE", mode)
    monkeypatch.setattr(S, "install", install_unfused if mode == "eager" else install_folded)
    monkeypatch.setattr(ops, "FusedErrorWatch", NoWatch)
    try:
        tools = cases.build_tools("tiny", qk_gain=R.QK_GAIN)
        return pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()),
                                   input_prompt=cases.RUNNER_PROMPT, num_inference_steps=steps, guidance_scale=R.GUIDANCE, seed=0, device="cpu",
                                   weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True, **kw)
    finally:
        uninstall_all()


@pytest.mark.parametrize("mode", ["eager", "folded"])
def test_host_layers_of_the_loop_match_the_oracle_loop(cpu_regions, monkeypatch, oracle_loops, mode):
    """Entry point, conditioning, _fold_regions and sampler on the CPU in fp32 (attention and mask launches replaced by restatements): the
    final latent of a 3-step request with the fixture is the oracle loop's. Bounds as in tests/test_negative_regions_host.py: eager runs the
    same fp32 ops in the same order (1e-6); folded runs the UNet at batch K + 2 = 7, whose GEMM / convolution summation order differs from
    batch 1 -- fp32 rounding through ~100 layers and 3 guided steps: 1e-4."""
    from gpu_util import rel_l2
    got = _host_loop(monkeypatch, mode, region_prompts=dict(R.REGIONS))
    d, visible = rel_l2(got, oracle_loops[(3, True)]), rel_l2(got, oracle_loops[(3, False)])
    print("%s host layers vs oracle loop: rel-L2 %.3e (against the loop without regions: %.3e)" % (mode, d, visible))
    assert d <= (1e-6 if mode == "eager" else 1e-4)
    assert visible > 1e-2


@pytest.mark.parametrize("off", [None, {}])
def test_default_takes_todays_path(cpu_regions, monkeypatch, off):
    """None and {}: _fold_regions is never reached, the folded dict is key by key what _fold_context builds today, the sampler is called
    without the new argument, and the latent is the same bits as without the keywords."""
    from pww_hip import sampler as S
    seen = []
    real = S._fold_context

    def spy(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]

    def never(*a, **kw):
        raise AssertionError("_fold_regions reached without region prompts")

    monkeypatch.setattr(S, "_fold_context", spy)
    monkeypatch.setattr(S, "_fold_regions", never)
    monkeypatch.setattr(S.ops, "region_combine", never)
    monkeypatch.setattr(S, "region_blend_fp32", never)
    plain = _host_loop(monkeypatch, "folded", steps=2)
    got = _host_loop(monkeypatch, "folded", steps=2, region_prompts=off, region_base_weight=0.5, region_feather=2.0)
    assert torch.equal(got, plain) and len(seen) == 2
    a, b = seen
    assert list(a) == list(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]) and a[k].shape == b[k].shape, k
        elif isinstance(a[k], int):
            assert a[k] == b[k], k
    assert tuple(a["CONTEXT_TENSOR"].shape[:2]) == (2, 77) and a["_PWW_ROW_GATE"].tolist() == [1.0, 0.0] and a["_PWW_GATED_ROWS"] == 1
