"""Negative regions, host side (no GPU): the `negative_color_context` / `negative_strength` keywords, the grammar of the negative dict, the
unconditional context dict it produces, the folded context of a CFG batch whose unconditional rows are biased too, and chunked prompts.

The mask kernels are replaced by the oracle's bilinear / blur restatements here (the launches themselves are pinned bit for bit on the
device: tests/test_negative_regions_gpu.py); what these tests look at is everything around them -- which phrases land in which columns of
which prompt, which keys and shapes the dicts carry -- against `oracle.pww_oracle.encode_text_color_inputs` called with
(negative_color_context, unconditional_input_prompt), whose `cond` dict IS the unconditional dict of the protocol."""
import importlib
import inspect

import numpy as np
import pytest
import torch

import pww_cases as cases
from host_standins import cpu_masks  # noqa: F401  (fixture)
from oracle import pww_oracle as O

SIDE = 64                                        # color map side: 64 / 16 / 4 / 1 tokens at ratios 8 / 16 / 32 / 64
KEYS = (64, 16, 4, 1)
WEIGHT_KEYS = ["CROSS_ATTENTION_WEIGHT_%d" % k for k in KEYS]
NEG_PROMPT = "blurry, a tree, low quality, a red car"
POS_CONTEXT = {(0, 0, 0): "cat,1.0", (255, 255, 255): "dog,1.5"}
POS_PROMPT = "a photo of a cat and a dog"


def _color_map():
    img = np.zeros((SIDE, SIDE, 3), dtype=np.uint8)                 # left half (0, 0, 0), right half white, a green square in the middle
    img[:, SIDE // 2:] = 255
    img[24:40, 24:40] = (13, 255, 0)
    return img


def _tools():
    from sd_standin import HashTokenizer, TinyTextEncoder
    return TinyTextEncoder(32, seed=1235), HashTokenizer()


def _encode(neg, uncond_prompt=NEG_PROMPT, pos=None, prompt=POS_PROMPT, **kw):
    from pww_hip.conditioning import _encode_text_color_inputs
    text, tok = _tools()
    return _encode_text_color_inputs(text, tok, "cpu", _color_map(), dict(POS_CONTEXT) if pos is None else pos, prompt, uncond_prompt,
                                     negative_color_context=neg, **kw)


def _entry_points():
    pw = importlib.import_module("paint_with_words.paint_with_words")
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    return [pw.paint_with_words, pw.paint_with_words_batch, inp.paint_with_words_inpaint, inp.paint_with_words_inpaint_batch]


def test_keywords_on_the_four_entry_points_and_the_pipeline_attributes():
    for f in _entry_points():
        params = inspect.signature(f).parameters
        names = list(params)
        assert params["negative_color_context"].default is None and params["negative_strength"].default == 1.0, f.__qualname__
        # extensions: behind every parameter of the reference (the last of them is `strength`)
        assert names.index("negative_color_context") > names.index("strength") and names.index("negative_strength") > names.index("strength")
    pipes = importlib.import_module("paint_with_words.pipelines")
    for cls in (pipes.PaintWithWord_StableDiffusionPipeline, pipes.PaintWithWord_StableDiffusionInpaintPipeline):
        assert cls.negative_color_context is None and cls.negative_strength == 1.0
        assert "negative_color_context" not in inspect.signature(cls.__call__).parameters


def test_a_seed_in_a_negative_entry_raises_before_anything_else():
    from pww_hip import conditioning as C
    eps = _entry_points()
    seeded = {(13, 255, 0): "a tree,1.0,2077"}
    for f, args in ((eps[0], ()), (eps[1], ({}, None, "", [0])), (eps[2], ()), (eps[3], ({}, None, None, None, "", [0]))):
        with pytest.raises(ValueError, match="seed"):
            f(*args, negative_color_context=dict(seeded))
        with pytest.raises(ValueError, match="negative_strength"):
            f(*args, negative_strength=float("nan"))
    with pytest.raises(ValueError, match="seed"):
        eps[1]({}, None, "", [0, 1], negative_color_context=[None, {(1, 2, 3): "x,1.0,7,2.5"}])
    kept = dict(seeded)
    with pytest.raises(ValueError):
        C.check_negative_context(kept)
    assert kept == seeded                                               # the check leaves the caller's dict alone
    C.check_negative_context({(13, 255, 0): "a tree,1.0,-1", (1, 2, 3): "x,0.5,-1,3.0"})      # -1: "no seed", as on the positive side
    pipes = importlib.import_module("paint_with_words.pipelines")
    for cls in (pipes.PaintWithWord_StableDiffusionPipeline, pipes.PaintWithWord_StableDiffusionInpaintPipeline):
        pipe = cls.__new__(cls)
        pipe.negative_color_context = dict(seeded)
        with pytest.raises(ValueError, match="seed"):
            pipe("a prompt", **({"image": 0, "mask_image": 0} if "Inpaint" in cls.__name__ else {}))


def test_grammar_strength_sigma_warning_and_stripping(cpu_masks, capsys):
    """Strength and blur sigma are honoured, a phrase that is not in the UNCONDITIONAL prompt warns like the positive side, and the caller's
    dict loses its tails -- expected maps: the oracle's builder on (negative_color_context, unconditional prompt)."""
    text, tok = _tools()
    neg = {(13, 255, 0): "a tree,1.5,-1,2.5", (255, 255, 255): "a red car,0.5", (0, 0, 0): "cat,1.0"}
    want_ctx = dict(neg)
    _, _, cond, uncond = _encode(neg)
    out = capsys.readouterr().out
    # "cat" is in the prompt, not in the unconditional prompt: one warning per missing phrase, in the positive side's words
    cat = tok("cat", max_length=77, truncation=True)["input_ids"][1:-1]
    assert out.count("Warning ratio 8 : tokens %s not found in text" % cat) == 1 and out.count("not found in text") == 1
    assert neg == {(13, 255, 0): "a tree,1.5", (255, 255, 255): "a red car,0.5", (0, 0, 0): "cat,1.0"}
    _, _, want, _ = O.encode_text_color_inputs(text, tok, _color_map(), want_ctx, NEG_PROMPT, "")
    from pww_hip.conditioning import PwWContext
    assert isinstance(uncond, PwWContext) and uncond.pending("CROSS_ATTENTION_WEIGHT_ORIG")
    assert [k for k in uncond if k.startswith("CROSS")] == WEIGHT_KEYS
    for key in WEIGHT_KEYS:
        assert uncond[key].dtype == torch.float32 and torch.equal(uncond[key], want[key]), key
    assert torch.equal(uncond["CROSS_ATTENTION_WEIGHT_ORIG"], want["CROSS_ATTENTION_WEIGHT_ORIG"])       # built on first access
    torch.testing.assert_close(uncond["CONTEXT_TENSOR"], want["CONTEXT_TENSOR"])
    # the blur reached the map: the tree's column is non-zero just outside its square (cell (2, 2) samples pixel (18, 18), the square starts at 24)
    ids = tok([NEG_PROMPT], padding="max_length", max_length=77, truncation=True, return_tensors="pt")["input_ids"][0].tolist()
    tree = tok("a tree", max_length=77, truncation=True)["input_ids"][1:-1]
    col = [i for i in range(77) if ids[i:i + len(tree)] == tree][0]
    w64 = uncond["CROSS_ATTENTION_WEIGHT_64"].reshape(8, 8, 77)
    assert float(w64[2, 2, col]) > 0.0 and float(w64[3, 3, col]) > float(w64[2, 2, col])
    # its own column bound: the last covered position of the unconditional prompt, rounded up to 16
    nz = [c for c in range(77) if float(uncond["CROSS_ATTENTION_WEIGHT_64"][:, c].abs().sum()) > 0]
    assert uncond["_PWW_BIAS_COLS"] == (max(nz) + 16) // 16 * 16 == 16
    # the positive side is what it was: same maps as without a negative context
    _, _, cond0, _ = _encode(None)
    for key in WEIGHT_KEYS:
        assert torch.equal(cond[key], cond0[key])
    # the pipeline classes parse the sigma and drop it, on this side too
    _, _, _, unc_ns = _encode({(13, 255, 0): "a tree,1.5,-1,2.5"}, use_sigma=False)
    _, _, want_ns, _ = O.encode_text_color_inputs(text, tok, _color_map(), {(13, 255, 0): "a tree,1.5,-1,2.5"}, NEG_PROMPT, "", use_sigma=False)
    assert torch.equal(unc_ns["CROSS_ATTENTION_WEIGHT_64"], want_ns["CROSS_ATTENTION_WEIGHT_64"])
    assert float(unc_ns["CROSS_ATTENTION_WEIGHT_64"].reshape(8, 8, 77)[2, 2, col]) == 0.0


@pytest.mark.parametrize("neg", [None, {}])
def test_default_takes_todays_path(cpu_masks, neg):
    """None and {}: the unconditional dict and the folded context are, key for key and shape for shape, what they are without the feature."""
    from pww_hip.sampler import _fold_context
    from pww_hip.conditioning import PwWContext
    _, _, cond, uncond = _encode(neg)
    assert type(uncond) is dict
    assert list(uncond) == ["CONTEXT_TENSOR", "CROSS_ATTENTION_WEIGHT_ORIG"] + WEIGHT_KEYS
    assert all(uncond[k] == 0 and isinstance(uncond[k], int) for k in uncond if k != "CONTEXT_TENSOR")
    assert tuple(uncond["CONTEXT_TENSOR"].shape) == (1, 77, 32)
    assert list(cond) == ["CONTEXT_TENSOR"] + WEIGHT_KEYS + ["_PWW_BIAS_COLS"] and cond["_PWW_BIAS_COLS"] == 16
    # shared maps: they stay [N, 77], the gate is [1, 1, 0, 0], the hint is n, nothing else is added
    f = _fold_context(cond, uncond, 2, "cpu")
    assert isinstance(f, PwWContext) and f.pending("CROSS_ATTENTION_WEIGHT_ORIG")
    assert list(f) == ["CONTEXT_TENSOR"] + WEIGHT_KEYS + ["_PWW_BIAS_COLS", "_PWW_KV_CACHE", "_PWW_ROW_GATE", "_PWW_GATED_ROWS"]
    assert f["_PWW_ROW_GATE"].tolist() == [1.0, 1.0, 0.0, 0.0] and f["_PWW_GATED_ROWS"] == 2 and f["_PWW_BIAS_COLS"] == 16
    assert tuple(f["CONTEXT_TENSOR"].shape) == (4, 77, 32)
    for k, key in zip(KEYS, WEIGHT_KEYS):
        assert f[key] is cond[key] and tuple(f[key].shape) == (k, 77)
    # per-image maps: [2n, 1, N, 77] with zeros for the unconditional rows
    _, _, cond_b, uncond_b = _encode(neg, pos={(0, 0, 0): "dog,0.7"})
    g = _fold_context([cond, cond_b], [uncond, uncond_b], 2, "cpu")
    assert list(g) == list(f)
    assert g["_PWW_ROW_GATE"].tolist() == [1.0, 1.0, 0.0, 0.0] and g["_PWW_GATED_ROWS"] == 2
    for k, key in zip(KEYS, WEIGHT_KEYS):
        assert tuple(g[key].shape) == (4, 1, k, 77) and float(g[key][2:].abs().sum()) == 0.0 and torch.equal(g[key][1, 0], cond_b[key])
    # the sampler's hipGraph signature keys on exactly these shapes and ints: literal
    sig = sorted((k, tuple(v.shape)) for k, v in f.items() if torch.is_tensor(v))
    assert sig == sorted([("CONTEXT_TENSOR", (4, 77, 32)), ("_PWW_ROW_GATE", (4,))] + [(key, (k, 77)) for k, key in zip(KEYS, WEIGHT_KEYS)])
    assert sorted((k, v) for k, v in f.items() if isinstance(v, int)) == [("_PWW_BIAS_COLS", 16), ("_PWW_GATED_ROWS", 2)]


def test_folded_context_with_negative_maps(cpu_masks):
    from pww_hip.sampler import _fold_context, _has_negative_maps
    from pww_hip.attention import ROW_GATE, GATED_ROWS, COND_ROWS, BIAS_COLS
    # the negative phrase sits behind position 16 of the unconditional prompt: the bound of the folded call is the negative side's
    far = "low quality, blurry, ugly, bad anatomy, watermark, text, signature, jpeg artifacts, worst quality, a tree"
    _, _, cond, uncond = _encode({(13, 255, 0): "a tree,1.0"}, uncond_prompt=far)
    assert _has_negative_maps(uncond) and not _has_negative_maps(_encode(None)[3])
    assert cond[BIAS_COLS] == 16 and uncond[BIAS_COLS] == 32
    f = _fold_context(cond, uncond, 2, "cpu", negative_strength=0.5)
    assert f[ROW_GATE].tolist() == [1.0, 1.0, 0.5, 0.5] and f[ROW_GATE].dtype == torch.float32
    assert f[GATED_ROWS] == 0 and f[COND_ROWS] == 2 and f[BIAS_COLS] == 32
    assert tuple(f["CONTEXT_TENSOR"].shape) == (4, 77, 32)
    for k, key in zip(KEYS, WEIGHT_KEYS):      # shared maps are materialised: the two halves differ
        assert tuple(f[key].shape) == (4, 1, k, 77)
        assert torch.equal(f[key][0, 0], cond[key]) and torch.equal(f[key][1, 0], cond[key])
        assert torch.equal(f[key][2, 0], uncond[key]) and torch.equal(f[key][3, 0], uncond[key])
    assert f.pending("CROSS_ATTENTION_WEIGHT_ORIG")
    orig = f["CROSS_ATTENTION_WEIGHT_ORIG"]
    assert tuple(orig.shape) == (4, SIDE, SIDE, 77) and torch.equal(orig[3], uncond["CROSS_ATTENTION_WEIGHT_ORIG"]) and torch.equal(orig[0], cond["CROSS_ATTENTION_WEIGHT_ORIG"])
    assert _fold_context(cond, uncond, 2, "cpu")[ROW_GATE].tolist() == [1.0, 1.0, 1.0, 1.0]       # negative_strength defaults to 1
    # per-image negative maps; a request of the batch without a negative context carries zero maps (negative_maps=True)
    _, _, cond_b, uncond_b = _encode(None, uncond_prompt=far, negative_maps=True)
    assert _has_negative_maps(uncond_b) and uncond_b[BIAS_COLS] == 16 and float(uncond_b["CROSS_ATTENTION_WEIGHT_64"].abs().sum()) == 0.0
    g = _fold_context([cond, cond_b], [uncond, uncond_b], 2, "cpu", negative_strength=2.0)
    assert g[ROW_GATE].tolist() == [1.0, 1.0, 2.0, 2.0] and g[GATED_ROWS] == 0 and g[COND_ROWS] == 2 and g[BIAS_COLS] == 32
    for k, key in zip(KEYS, WEIGHT_KEYS):
        assert tuple(g[key].shape) == (4, 1, k, 77) and torch.equal(g[key][2, 0], uncond[key]) and float(g[key][3].abs().sum()) == 0.0
    # a batch that mixes the reference's integer slots with negative maps cannot be stacked
    with pytest.raises(ValueError, match="negative regions"):
        _fold_context([cond, cond_b], [uncond, _encode(None)[3]], 2, "cpu")
    # same geometry, other maps: the sampler's signature (shapes and ints) is the same -- one captured graph serves both
    _, _, cond2, uncond2 = _encode({(255, 255, 255): "a tree,0.3"}, uncond_prompt=far)
    f2 = _fold_context(cond2, uncond2, 2, "cpu", negative_strength=0.25)
    # (the sampler leaves the full-resolution fallback map out of the signature: it exists only once a layer asked for it)
    shape_sig = lambda d: sorted((k, tuple(v.shape)) for k, v in d.items() if torch.is_tensor(v) and not k.endswith("_ORIG"))      # noqa: E731
    int_sig = lambda d: sorted((k, v) for k, v in d.items() if isinstance(v, int))                    # noqa: E731
    assert shape_sig(f2) == shape_sig(f) and int_sig(f2) == int_sig(f) and not torch.equal(f2[WEIGHT_KEYS[0]], f[WEIGHT_KEYS[0]])
    f0 = _fold_context(*_encode(None, uncond_prompt=far)[2:], 2, "cpu")
    assert (shape_sig(f0), int_sig(f0)) != (shape_sig(f), int_sig(f))                                   # switching negatives on / off re-captures


def test_recorder_records_the_conditional_rows_only(monkeypatch):
    """The hint says 0 ("every row is biased"), the recorder still gets exactly the n conditional rows."""
    from pww_hip import attention, attnmaps, ops
    seen = {}
    monkeypatch.setattr(ops, "attention_probs", lambda q, k, heads, scale, **kw: seen.update(kw))
    rec = attnmaps.AttentionRecorder()
    rec.begin_request(3)
    rec._live[16] = torch.zeros(3, 16, 77)       # (the accumulator of the 16-token layers: allocated by the first call on a device)
    q, k = torch.zeros(6, 16, 64), torch.zeros(6, 77, 64)
    attn = type("A", (), {"heads": 2, "scale": 1.0})()
    gate = torch.tensor([1.0, 1.0, 1.0, 0.5, 0.5, 0.5])
    ctx = {attention.ROW_GATE: gate, attention.GATED_ROWS: 0, attention.COND_ROWS: 3}
    attention._record_probs(rec, attn, ctx, q, k, torch.zeros(6, 1, 16, 77), gate, None, None)
    assert seen["images"] == 3 and tuple(seen["out"].shape) == (3, 16, 77)
    # without negatives the hint itself says which rows are conditional, as before
    seen.clear()
    attention._record_probs(rec, attn, {attention.ROW_GATE: gate, attention.GATED_ROWS: 3}, q, k, None, None, None, None)
    assert seen["images"] == 3


def test_chunked_prompts_negative_phrase_across_a_boundary(cpu_masks, capsys):
    from pww_hip import conditioning as C
    text, tok = _tools()
    words = lambda n, stem="word": " ".join("%s%d" % (stem, i) for i in range(n))      # noqa: E731
    # a 160-token unconditional prompt under a short prompt: the request is encoded to the 3 chunks the unconditional prompt needs
    neg = {(13, 255, 0): "neg74 neg75 neg76,1.0", (255, 255, 255): "neg150,0.5"}
    _, _, cond, uncond = _encode(dict(neg), uncond_prompt=words(160, "neg"), max_prompt_chunks=3)
    assert "not found" not in capsys.readouterr().out
    assert tuple(cond["CONTEXT_TENSOR"].shape) == (1, 231, 32) and tuple(uncond["CONTEXT_TENSOR"].shape) == (1, 231, 32)
    w = uncond["CROSS_ATTENTION_WEIGHT_64"]
    assert tuple(w.shape) == (64, 231) and tuple(cond["CROSS_ATTENTION_WEIGHT_64"].shape) == (64, 231)
    assert [c for c in range(231) if float(w[:, c].abs().sum()) > 0] == [75, 78, 79, 155]      # content 74 | 75, 76 straddle the first boundary
    assert uncond["_PWW_BIAS_COLS"] == 160
    # expected values: the oracle's map over the UNFRAMED ids, scattered to the framed columns
    ids = C._content_ids(tok, words(160, "neg"))
    regions, _, _ = O.separate_regions(_color_map(), dict(neg), tok)
    flat = torch.from_numpy(O.tokens_img_attention_weight(regions, ids, 8))
    for p in (74, 75, 76, 150, 0, 149):
        assert torch.equal(w[:, C.framed_column(p)], flat[:, p])
    # the cap holds for both prompts; under cap 2 the third chunk's phrase is cut and warned about
    _, _, cond2, uncond2 = _encode(dict(neg), uncond_prompt=words(160, "neg"), max_prompt_chunks=2)
    assert capsys.readouterr().out.count("not found in text") == 1
    assert tuple(cond2["CONTEXT_TENSOR"].shape) == (1, 154, 32) and tuple(uncond2["CROSS_ATTENTION_WEIGHT_64"].shape) == (64, 154)
    # the larger of the two counts, whichever prompt is the long one; the default cap keeps one chunk
    _, _, cond3, uncond3 = _encode({(13, 255, 0): "a tree,1.0"}, prompt=words(100) + " a cat", max_prompt_chunks=3)
    assert tuple(cond3["CONTEXT_TENSOR"].shape) == (1, 154, 32) and tuple(uncond3["CROSS_ATTENTION_WEIGHT_16"].shape) == (16, 154)
    _, _, cond1, uncond1 = _encode(dict(neg), uncond_prompt=words(60, "neg"))
    assert tuple(cond1["CONTEXT_TENSOR"].shape) == (1, 77, 32) and tuple(uncond1["CROSS_ATTENTION_WEIGHT_64"].shape) == (64, 77)
    pw = importlib.import_module("paint_with_words.paint_with_words")
    assert pw._batch_prompt_chunks(tok, [words(10), words(100)] + [words(160, "neg")], 3) == 3


def test_batch_forms_share_or_split_the_negative_context():
    pw = importlib.import_module("paint_with_words.paint_with_words")
    one = {(1, 2, 3): "a tree,1.0"}
    assert pw._broadcast(one, 3, "negative_color_context") == ([one] * 3, True)
    assert pw._broadcast(None, 2, "negative_color_context") == ([None, None], True)
    per, shared = pw._broadcast([one, None, {}], 3, "negative_color_context")
    assert not shared and per == [one, None, {}]
    with pytest.raises(ValueError, match="negative_color_context has 2 entries"):
        pw._broadcast([one, None], 3, "negative_color_context")
    maps = [object()] * 3
    assert pw._negative_contexts([one, None, {}], 3, maps) == ([one, None, None], True)
    assert pw._negative_contexts(None, 2, maps) == ([None, None], False) and pw._negative_contexts([{}, None], 2, maps) == ([None, None], False)
    assert pw._negative_contexts([one], 1, [None]) == ([None], False)        # no color map: no regions on either side


def test_request_broadcast_carries_the_negative_context(tmp_path):
    """pww_hip.dist.broadcast_request through a real (one-rank, gloo) process group: the negative context -- tuple keys, tails and all --
    and the strength come out of the pickled part of the payload as they went in, beside the color map's array. The broadcast needed no
    code for this (it pickles every non-array entry), so this test passes without the feature too: it pins the property the feature relies on."""
    import torch.distributed as dist
    from pww_hip import dist as pdist
    payload = {"rgb": _color_map(), "context": dict(POS_CONTEXT), "prompt": POS_PROMPT, "negative_context": {(13, 255, 0): "a tree,1.0,-1,2.5"},
               "negative_strength": 0.5}
    dist.init_process_group(backend="gloo", init_method="file://%s" % (tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        got = pdist.broadcast_request(payload, "cpu")
    finally:
        dist.destroy_process_group()
    assert got is not payload and set(got) == set(payload)
    assert got["negative_context"] == {(13, 255, 0): "a tree,1.0,-1,2.5"} and got["negative_strength"] == 0.5
    assert np.array_equal(got["rgb"], _color_map())


# ---- the loop's host layers against the oracle loop, on the CPU ----------------------------------------------------------------------

def _folded_forward(module, hidden_states, context=None, mask=None):
    """fp32 torch restatement of what the cross-attention launches compute for a (folded) dict context: per image b,
    bias_b = gate[b] * weight_function(w_b, sigma, scores_b) with the image's own scores, added before the scale."""
    from pww_hip.attention import ROW_GATE
    if not isinstance(context, dict):
        return O.inj_forward(module, hidden_states, context)
    h, ctx, gate = module.heads, context["CONTEXT_TENSOR"], context.get(ROW_GATE)
    outs = []
    for b in range(hidden_states.shape[0]):
        q, k, v = (O.split_heads(torch.nn.functional.linear(x[b:b + 1], m.weight), h)
                   for x, m in ((hidden_states, module.to_q), (ctx, module.to_k), (ctx, module.to_v)))
        scores = torch.matmul(q, k.transpose(-1, -2))
        w = context["CROSS_ATTENTION_WEIGHT_%d" % scores.shape[-2]]
        if torch.is_tensor(w) and w.dim() == 4:
            w = w[b, 0]
        bias = context["WEIGHT_FUNCTION"](w, context["SIGMA"], scores)
        if gate is not None:
            bias = bias * gate[b]
        outs.append(O.merge_heads(torch.matmul(((scores + bias) * module.scale).softmax(dim=-1), v), h))
    return torch.nn.functional.linear(torch.cat(outs), module.to_out[0].weight, module.to_out[0].bias)


@pytest.fixture(scope="module")
def oracle_loops():
    import negative_cases as G
    return G, {(steps, on): G.oracle_loop(G.NEG_CONTEXT if on else None, G.NEG_STRENGTH, steps=steps) for steps, on in ((3, True), (10, True), (10, False))}


def test_fixture_is_visible_in_the_oracle(oracle_loops):
    """The fixture of tests/negative_cases.py moves the oracle's final latent by at least twice the widest cap the HIP path is
    held to there (bf16: 1e-1); profiles/negative_regions.md records 0.562."""
    G, lat = oracle_loops
    from gpu_util import rel_l2
    d = rel_l2(lat[(10, True)], lat[(10, False)])
    print("oracle: rel-L2(with negative context, without) = %.3e" % d)
    assert d >= 2 * G.CAP[torch.bfloat16]
    assert abs(d - G.ORACLE_VISIBLE) <= 0.1 * G.ORACLE_VISIBLE


@pytest.mark.parametrize("mode", ["eager", "folded"])
def test_host_layers_of_the_loop_match_the_oracle_loop(cpu_masks, monkeypatch, oracle_loops, mode):
    """Entry point, conditioning, _fold_context and sampler on the CPU in fp32, with the attention launches replaced by torch restatements
    (eager: the reference's op sequence per batch-1 call, gpu_util.unfused_inj_forward; folded: _folded_forward above) and the mask launches
    by the oracle's resize: the final latent of a 3-step request with the negative fixture is the oracle loop's. Bounds: eager runs the same
    fp32 ops in the same order (1e-6); folded runs the UNet at batch 2, whose GEMM / convolution summation order differs from batch 1 --
    fp32 rounding (1.2e-7) through ~100 layers and 3 guided steps: 1e-4. (profiles/negative_regions.md: measured 0 and 3.0e-6.)"""
    from PIL import Image
    import paint_with_words as pw
    from gpu_util import install_unfused, uninstall_all, rel_l2
    from pww_hip import ops, sampler as S
    G, lat = oracle_loops
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")

    def install_folded(unet):
        for m in unet.modules():
            if m.__class__.__name__ == "CrossAttention":
                m.__class__.__call__ = _folded_forward

    class NoWatch:      # (the hand-off error words live on the device)
        def poll(self, wait=False):
            pass

        def post(self, modules):
            return False

    monkeypatch.setattr(pww_mod, "DEFAULT_MODE", mode)
    monkeypatch.setattr(S, "install", install_unfused if mode == "eager" else install_folded)
    monkeypatch.setattr(ops, "FusedErrorWatch", NoWatch)
    try:
        tools = cases.build_tools("tiny", qk_gain=G.QK_GAIN)
        got = pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()),
                                  input_prompt=cases.RUNNER_PROMPT, num_inference_steps=3, guidance_scale=7.5, seed=0, device="cpu",
                                  weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True,
                                  unconditional_input_prompt=G.NEG_PROMPT, negative_color_context=dict(G.NEG_CONTEXT), negative_strength=G.NEG_STRENGTH)
    finally:
        uninstall_all()
    d = rel_l2(got, lat[(3, True)])
    print("%s host layers vs oracle loop: rel-L2 %.3e" % (mode, d))
    assert d <= (1e-6 if mode == "eager" else 1e-4)
