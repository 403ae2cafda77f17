"""Host side of the CLIP text encoder route: the side library's table rows, a real build with its argument checks, the stand-in against
transformers' CLIPTextModel, the route's structural check, and that an encoder the route does not cover is called exactly as before. No GPU."""
import ctypes
import inspect
import subprocess

import pytest
import torch
import torch.nn as nn

import text_cases as tc
from conftest import PKG, REPO


# ---- the table pair ------------------------------------------------------------------------------------------------------------------------
def test_the_table_row_header_and_exports(built_lib):
    import build as pww_build
    from pww_hip import _lib
    assert tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA) and tuple(_lib.SIDE_EXTRA)[-1] == "text"
    spec = _lib.side_spec("text")
    assert spec is _lib.SIDE_EXTRA["text"] and set(spec) == set(_lib.SIDE["regions"]) and spec["missing_ok"] is False
    assert spec["exports"] is _lib.TEXT_EXPORTS and spec["min_version"] == _lib.TEXT_MIN_VERSION == 100 and spec["path"] == "TEXT_LIB_PATH"
    assert _lib.TEXT_LIB_PATH.endswith("libpww_hip_text.so") and "PWW_HIP_TEXT_LIB" in inspect.getsource(_lib)
    assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_text_version", "pww_text_last_error"}
    assert set(spec["exports"]) == {"pww_text_version", "pww_text_last_error", "pww_text_embed_ln", "pww_text_attn_fwd", "pww_text_act"}
    assert callable(_lib.load_text) and callable(pww_build.build_text)
    assert pww_build.SIDE_LIBS_EXTRA["text"][0] == "pww_text.hip" and pww_build.TEXT_UNITS == [("pww_text.hip", ["-fvisibility=hidden"], "")]
    assert pww_build.LIB_TEXT == pww_build.SIDE_PATHS["text"] and "text " in pww_build.__doc__ and "Fifteen libraries" in pww_build.__doc__
    header = open(REPO + "/include/pww_hip_text.h").read()
    for line in ("#define PWW_TEXT_VERSION 100", "#define PWW_TEXT_HEAD_DIM 64", "#define PWW_TEXT_MAX_TOKENS 128", "#define PWW_TEXT_ACT_QUICK_GELU 0",
                 "#define PWW_TEXT_ACT_GELU 1"):
        assert line in header, line
    assert (_lib.TEXT_HEAD_DIM, _lib.TEXT_MAX_TOKENS, _lib.TEXT_ACT_QUICK_GELU, _lib.TEXT_ACT_GELU) == (64, 128, 0, 1)
    for fn in spec["exports"]:
        assert "%s(" % fn in header
    source = open(PKG + "/csrc/pww_text.hip").read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_text"' in source
    assert "atomic" not in source
    # the linear library is as it was
    assert _lib.LINEAR_MIN_VERSION == 100 and "#define PWW_LINEAR_VERSION 100" in open(REPO + "/include/pww_hip_linear.h").read()


def test_a_real_load_binds_the_entry_points_and_checks_arguments_on_the_host(built_lib):
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_text()
    lib = _lib.load_side("text")
    assert lib is not None and _lib.load_text() is lib and lib.pww_text_version() == 100
    for fn, (argtypes, restype) in _lib.SIDE_EXTRA["text"]["sigs"].items():
        assert getattr(lib, fn).argtypes == argtypes and getattr(lib, fn).restype is restype, fn
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.TEXT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in dyn.splitlines() if " T " in line and not line.split()[-1].startswith(("_init", "_fini")))
    assert visible == sorted(_lib.TEXT_EXPORTS)             # -fvisibility=hidden: the entry points and nothing else
    one = ctypes.c_void_p(16)           # (never dereferenced: every call below is refused before the first HIP call)
    bf = _lib.DTYPE_BF16

    def embed(ids=one, tok=one, x=one, R=1, L=77, C=768, V=1000, P=77, eps=1e-5, dtype=bf):
        return lib.pww_text_embed_ln(ids, tok, one, one, one, x, one, R, L, C, V, P, eps, dtype, None)

    def attn(qkv=one, o=one, R=1, H=12, L=77, ld=2304, old=768, dtype=bf):
        return lib.pww_text_attn_fwd(qkv, o, R, H, L, ld, old, dtype, None)

    def act(x=one, M=77, N=3072, stride=3072, a=0, dtype=bf):
        return lib.pww_text_act(x, M, N, stride, a, dtype, None)
    # a null pointer: PWW_EINVAL, the library's own error slot says which call, nothing is launched
    for call, name in ((lambda: embed(ids=None), b"text_embed_ln"), (lambda: embed(x=None), b"text_embed_ln"), (lambda: attn(qkv=None), b"text_attn"),
                       (lambda: attn(o=None), b"text_attn"), (lambda: act(x=None), b"text_act")):
        assert call() == _lib.PWW_EINVAL
        msg = lib.pww_text_last_error()
        assert msg and name in msg and b"required" in msg
    # L = 0 is a size below 1 (PWW_EINVAL); L = 129, C = 96 and an unknown activation are shapes the library is not built for (PWW_ENOTSUP)
    assert attn(L=0) == _lib.PWW_EINVAL and b">= 1" in lib.pww_last_error()
    assert embed(L=0) == _lib.PWW_EINVAL and b">= 1" in lib.pww_last_error()
    assert attn(L=129) == _lib.PWW_ENOTSUP and b"at most 128" in lib.pww_last_error()
    assert embed(C=96) == _lib.PWW_ENOTSUP and b"multiple of 64" in lib.pww_last_error()
    assert act(a=2) == _lib.PWW_ENOTSUP and b"unknown activation" in lib.pww_last_error()
    # the rest of the documented refusals
    assert embed(L=78) == _lib.PWW_ENOTSUP and b"positions" in lib.pww_last_error()
    assert embed(dtype=2) == _lib.PWW_ENOTSUP and attn(dtype=2) == _lib.PWW_ENOTSUP and act(dtype=2) == _lib.PWW_ENOTSUP
    assert embed(eps=0.0) == _lib.PWW_ENOTSUP and embed(C=8192) == _lib.PWW_ENOTSUP
    assert attn(ld=2296) == _lib.PWW_ENOTSUP and attn(old=760) == _lib.PWW_ENOTSUP and attn(ld=2308) == _lib.PWW_ENOTSUP and b"strides" in lib.pww_last_error()
    assert attn(qkv=ctypes.c_void_p(8)) == _lib.PWW_ENOTSUP and b"aligned" in lib.pww_last_error()
    assert attn(R=6000) == _lib.PWW_ENOTSUP and b"65535" in lib.pww_last_error()
    assert act(N=60, stride=64) == _lib.PWW_ENOTSUP and act(stride=3064) == _lib.PWW_ENOTSUP and act(M=0) == _lib.PWW_EINVAL
    assert act(M=1 << 20, N=4096, stride=4096) == _lib.PWW_ENOTSUP and b"2^31" in lib.pww_last_error()


def test_a_missing_file_is_an_error(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "text", None)
    monkeypatch.setattr(_lib, "TEXT_LIB_PATH", str(tmp_path / "libpww_hip_text.so"))
    with pytest.raises(_lib.PwwHipError, match="libpww_hip_text.so not found .*rebuild"):
        _lib.load_text()


# ---- the stand-in --------------------------------------------------------------------------------------------------------------------------
def test_the_stand_in_is_built_under_a_restored_generator():
    from sd_standin import CLIPTextEncoder
    state = torch.random.get_rng_state()
    a = CLIPTextEncoder(vocab=100, **tc.TOPOLOGIES["tiny"])
    b = CLIPTextEncoder(vocab=100, **tc.TOPOLOGIES["tiny"])
    assert torch.equal(torch.random.get_rng_state(), state)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters())) and not any(p.requires_grad for p in a.parameters())
    assert not hasattr(a, "text_model") and a.config.num_attention_heads == 2 and a.config.hidden_act == "quick_gelu" and a.config.layer_norm_eps == 1e-5
    out = a(tc.prompt_ids(2, vocab=100))
    assert isinstance(out, tuple) and tuple(out[0].shape) == (2, 77, 128)
    with pytest.raises(ValueError):
        CLIPTextEncoder(vocab=100, ctx_dim=128, layers=1, heads=2, intermediate=256, hidden_act="relu")


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_the_stand_in_is_transformers_clip_text_model(act):
    transformers = pytest.importorskip("transformers")
    from sd_standin import CLIPTextEncoder
    cfg = transformers.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                      max_position_embeddings=77, hidden_act=act, bos_token_id=998, eos_token_id=999)
    state = torch.random.get_rng_state()
    torch.manual_seed(11)
    try:
        real = transformers.CLIPTextModel(cfg).eval().double()
    finally:
        torch.random.set_rng_state(state)
    sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in real.state_dict().items() if not k.endswith("position_ids")}
    mine = CLIPTextEncoder(vocab=1000, ctx_dim=128, layers=2, heads=2, intermediate=256, hidden_act=act).double().eval()
    assert set(sd) == set(mine.state_dict())                # the same keys: the 5.x layout (or 4.x's without its prefix)
    mine.load_state_dict(sd)
    ids = tc.prompt_ids(3, vocab=1000)
    with torch.no_grad():
        want = real(ids)[0]
        got = mine(ids)[0]
    peak = want.abs().max().item()
    # fp64 round-off over two layers
    assert (got - want).abs().max().item() <= 1e-9 * peak
    assert (tc.reference(mine, ids) - got).abs().max().item() <= 1e-9 * peak


# ---- covers --------------------------------------------------------------------------------------------------------------------------------
class _Wrapped(nn.Module):
    """The transformers 4.x form: the model under .text_model."""
    def __init__(self, inner):
        super().__init__()
        self.text_model, self.config = inner, inner.config

    def forward(self, ids):
        return self.text_model(ids)


def _standin(dtype=torch.bfloat16, **over):
    from sd_standin import CLIPTextEncoder
    kw = dict(tc.TOPOLOGIES["tiny"], vocab=100)
    kw.update(over)
    return CLIPTextEncoder(**kw).to(dtype)


def test_covers_is_a_structural_check():
    from pww_hip import text_encode as E
    from sd_standin import TinyTextEncoder
    for dtype in (torch.bfloat16, torch.float16):
        m = _standin(dtype)
        assert E.covers(m, require_device=False) and E.covers(_Wrapped(m), require_device=False)
        assert not E.covers(m) and not E.covers(_Wrapped(m))                     # on the CPU
    assert not E.covers(TinyTextEncoder(128), require_device=False) and not E.covers(TinyTextEncoder(128).to(torch.bfloat16), require_device=False)
    assert not E.covers(_standin(torch.float32), require_device=False)
    assert not E.covers(_standin(heads=4), require_device=False)                # head dim 32
    assert not E.covers(_standin(ctx_dim=2112, heads=33, layers=1), require_device=False)      # wider than ops.add_layer_norm takes (2048)
    relu = _standin()
    relu.config.hidden_act = "relu"
    assert not E.covers(relu, require_device=False)
    nobias = _standin()
    nobias.encoder.layers[1].mlp.fc1.bias = None
    assert not E.covers(nobias, require_device=False)
    mixed = _standin()
    mixed.final_layer_norm.float()
    assert not E.covers(mixed, require_device=False)
    assert not E.covers(None, require_device=False) and not E.covers(nn.Linear(4, 4), require_device=False)
    assert set(E.stats()) == {"embed", "attention", "act", "linear", "layer_norm", "encodes", "rows"}
    with pytest.raises(E.PwwHipError, match="covers"):
        E.encode(_standin(), tc.prompt_ids(1, vocab=100))                        # no quiet fall-back: a module that is not covered is an error


def test_the_switches_are_read_per_call(monkeypatch):
    from pww_hip import text_encode as E
    for name, fn in (("PWW_TEXT_ENCODE", E.enabled), ("PWW_TEXT_EMBED", E.embed_enabled), ("PWW_TEXT_ATTN", E.attn_enabled), ("PWW_TEXT_ACT", E.act_enabled)):
        monkeypatch.setenv(name, "0")
        assert fn() is False
        monkeypatch.setenv(name, "1")
        assert fn() is True
    monkeypatch.delenv("PWW_TEXT_ACT")
    assert E.act_enabled("quick_gelu") is True and E.act_enabled("gelu") is False          # gelu measured slower than F.gelu: off unless asked for
    monkeypatch.setenv("PWW_TEXT_ACT", "1")
    assert E.act_enabled("gelu") is True
    for value, want in (("0", "0"), ("force", "force"), ("1", "table"), ("", "table")):
        monkeypatch.setenv("PWW_TEXT_LINEAR", value)
        assert E.linear_mode() == want
    # the plan handed to ops.linear is a function of (K, N) alone
    assert E._gemm_plan(128, 384) == E._gemm_plan(128, 384) and "M" not in inspect.signature(E._gemm_plan).parameters
    for (K, N), (tile_n, splitk) in E.LINEAR_ROUTES.items():
        assert tile_n in (64, 128) and N % tile_n == 0 and 1 <= splitk <= K // 64


# ---- an encoder the route does not cover is called as before -----------------------------------------------------------------------------
class _Spy:
    def __init__(self, module):
        self.module, self.calls = module, []

    def __call__(self, ids):
        self.calls.append(ids.clone())
        return self.module(ids)


LONG = " ".join("word%d" % i for i in range(100))          # 100 content tokens: two chunks


def test_encode_rows_calls_a_tiny_encoder_row_by_row(monkeypatch):
    from pww_hip import conditioning as C, ops
    from pww_hip import text_encode as E
    from sd_standin import HashTokenizer, TinyTextEncoder
    te, tok = TinyTextEncoder(64), HashTokenizer()
    E.reset_stats()
    # the chunked site: cond rows, then uncond rows, a [1, 77] batch each
    spy = _Spy(te)
    _, _, cond, uncond = C._encode_text_color_inputs(spy, tok, "cpu", None, {}, LONG, "", max_prompt_chunks=2)
    _, rows = C.chunk_prompt(tok, LONG, 2, 1)
    _, urows = C.chunk_prompt(tok, "", 2, 2)
    assert len(rows) == 2 and len(spy.calls) == 4 and all(tuple(c.shape) == (1, 77) and c.dtype == torch.long for c in spy.calls)
    assert [c[0].tolist() for c in spy.calls] == rows + urows
    direct = lambda rr: torch.cat([te(torch.tensor([r], dtype=torch.long))[0] for r in rr], dim=1)      # noqa: E731
    assert tuple(cond["CONTEXT_TENSOR"].shape) == (1, 154, 64)
    assert torch.equal(cond["CONTEXT_TENSOR"], direct(rows)) and torch.equal(uncond["CONTEXT_TENSOR"], direct(urows))
    # the plain site: cond, then uncond
    spy = _Spy(te)
    _, _, cond, uncond = C._encode_text_color_inputs(spy, tok, "cpu", None, {}, "a cat", "blurry")
    want = [tok([p], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids for p in ("a cat", "blurry")]
    assert len(spy.calls) == 2 and all(torch.equal(c, w) for c, w in zip(spy.calls, want))
    assert torch.equal(cond["CONTEXT_TENSOR"], te(want[0])[0]) and torch.equal(uncond["CONTEXT_TENSOR"], te(want[1])[0])
    # the region-prompt site, one chunk and two (the masks are a GPU kernel: not what is under test here)
    monkeypatch.setattr(ops, "region_masks", lambda rgb, colors, feather=0.0: torch.zeros(len(colors), 8, 8))
    import numpy as np
    rgb = np.zeros((64, 64, 3), dtype=np.uint8)
    regions = {(255, 0, 0): "a red fox", (0, 255, 0): LONG}
    for k in (1, 2):
        like = {"CONTEXT_TENSOR": torch.zeros(1, 77 * k, 64), "CROSS_ATTENTION_WEIGHT_64": 0}
        spy = _Spy(te)
        plan = C.encode_region_prompts(spy, tok, "cpu", rgb, regions, 7.5, like)
        entries = C.region_entries(regions)
        if k == 1:
            want = [tok([e[1]], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids[0].tolist() for e in entries]
            per = [[w] for w in want]
        else:
            per = [C.chunk_prompt(tok, e[1], 2, 2)[1] for e in entries]
            want = [r for rr in per for r in rr]
        assert len(spy.calls) == 2 * k and all(tuple(c.shape) == (1, 77) for c in spy.calls) and [c[0].tolist() for c in spy.calls] == want
        for ctx, rr in zip(plan["contexts"], per):
            assert torch.equal(ctx["CONTEXT_TENSOR"], direct(rr)) and ctx["CROSS_ATTENTION_WEIGHT_64"] == 0
    # the helper itself: lists and tensors alike, [R, L, C]
    out = C.encode_rows(te, [rows[0], torch.tensor([rows[1]])], "cpu")
    assert tuple(out.shape) == (2, 77, 64) and torch.equal(out[1:], te(torch.tensor([rows[1]]))[0])
    st = E.stats()
    assert st["encodes"] == 0 and st["rows"] == 0 and all(st[p] == {"native": 0, "stock": 0} for p in E._PARTS)
