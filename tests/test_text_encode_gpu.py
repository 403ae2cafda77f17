"""pww_hip.text_encode.encode against the fp64 restatement of the CLIP text forward (text_cases.reference), in fp16 and bf16, under the bar of
text_cases.py with the stand-in module's own forward in that dtype on the GPU as the stock route; the counters, the switches, row independence,
the cached packed weight, and a whole request through conditioning.encode_rows."""
import copy

import pytest
import torch

import pww_cases as cases
import text_cases as tc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
SWITCHES = ("PWW_TEXT_ENCODE", "PWW_TEXT_EMBED", "PWW_TEXT_ATTN", "PWW_TEXT_ACT", "PWW_TEXT_LINEAR")


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _expected(E, module, mode="table"):
    """The counters of one default-route encode of `module`, from the module and the route table alone."""
    layers = list(module.encoder.layers)
    C, inner = module.config.hidden_size, module.config.intermediate_size
    shapes = [(C, 3 * C), (C, C), (C, inner), (inner, C)]
    native = len(layers) * (4 if mode == "force" else 0 if mode == "0" else sum(s in E.LINEAR_ROUTES for s in shapes))
    act = (len(layers), 0) if E.act_enabled(module.config.hidden_act) else (0, len(layers))      # (gelu ships off: it measured slower than F.gelu)
    return {"embed": (1, 0), "attention": (len(layers), 0), "act": act, "linear": (native, 4 * len(layers) - native),
            "layer_norm": (2 * len(layers), 0)}


def _as_pairs(st, E):
    return {p: (st[p]["native"], st[p]["stock"]) for p in E._PARTS}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("name", ["tiny", "sd15", "sd2"])
def test_encode_against_the_reference(gpu_device, name, R, dtype):
    from pww_hip import text_encode as E
    module = copy.deepcopy(tc.encoder(name, dtype)).to(gpu_device)
    ids, ref = tc.encoder_case(name, dtype, R)
    assert E.covers(module) and E.enabled()
    E.reset_stats()
    got = E.encode(module, ids)
    st = E.stats()
    with torch.no_grad():
        stock = module(ids.to(gpu_device))[0]
    assert got.dtype == dtype and tuple(got.shape) == (R, 77, module.config.hidden_size)
    tc.check(got, stock, ref, "encode %s R %d %s" % (name, R, dtype))
    # every part the defaults turn on ran native, once per place it occurs
    assert st["encodes"] == 1 and st["rows"] == R and _as_pairs(st, E) == _expected(E, module)
    assert torch.equal(got, E.encode(module, ids.to(gpu_device)))              # device ids; bitwise repeatable


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_runs_native_behind_its_switch(gpu_device, monkeypatch, dtype):
    from pww_hip import text_encode as E
    module = copy.deepcopy(tc.encoder("sd2", dtype)).to(gpu_device)
    ids, ref = tc.encoder_case("sd2", dtype, 1)
    assert E.act_enabled("quick_gelu") and not E.act_enabled("gelu")
    monkeypatch.setenv("PWW_TEXT_ACT", "1")
    E.reset_stats()
    got = E.encode(module, ids)
    assert E.stats()["act"] == {"native": 1, "stock": 0}
    with torch.no_grad():
        stock = module(ids.to(gpu_device))[0]
    tc.check(got, stock, ref, "encode sd2 %s PWW_TEXT_ACT=1" % dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_switches_and_counters(gpu_device, monkeypatch, dtype):
    from pww_hip import conditioning as C
    from pww_hip import text_encode as E
    module = copy.deepcopy(tc.encoder("tiny", dtype)).to(gpu_device)
    R = 3
    ids, ref = tc.encoder_case("tiny", dtype, R)
    with torch.no_grad():
        stock = module(ids.to(gpu_device))[0]
        per_row = torch.cat([module(ids[r:r + 1].to(gpu_device))[0] for r in range(R)], 0)
    base = _expected(E, module)
    n = len(module.encoder.layers)
    moved = {"PWW_TEXT_EMBED": ("embed", (0, 1)), "PWW_TEXT_ATTN": ("attention", (0, n)), "PWW_TEXT_ACT": ("act", (0, n))}
    for name, (part, want) in moved.items():
        monkeypatch.setenv(name, "0")
        E.reset_stats()
        got = E.encode(module, ids)
        monkeypatch.delenv(name)
        st = _as_pairs(E.stats(), E)
        assert st[part] == want and {k: v for k, v in st.items() if k != part} == {k: v for k, v in base.items() if k != part}, (name, st)
        tc.check(got, stock, ref, "encode tiny %s %s=0" % (dtype, name))
    for value in ("0", "force"):
        monkeypatch.setenv("PWW_TEXT_LINEAR", value)
        E.reset_stats()
        got = E.encode(module, ids)
        monkeypatch.delenv("PWW_TEXT_LINEAR")
        assert _as_pairs(E.stats(), E) == _expected(E, module, value), value
        tc.check(got, stock, ref, "encode tiny %s PWW_TEXT_LINEAR=%s" % (dtype, value))
    # PWW_TEXT_ENCODE=0: the helper makes the stock per-row calls and nothing is counted
    monkeypatch.setenv("PWW_TEXT_ENCODE", "0")
    E.reset_stats()
    rows = [ids[r:r + 1] for r in range(R)]
    got = C.encode_rows(module, rows, gpu_device)
    st = E.stats()
    assert st["encodes"] == 0 and st["rows"] == 0 and all(v == (0, 0) for v in _as_pairs(st, E).values())
    assert torch.equal(got, per_row)
    monkeypatch.delenv("PWW_TEXT_ENCODE")
    E.reset_stats()
    got = C.encode_rows(module, rows, gpu_device)
    assert E.stats()["encodes"] == 1 and E.stats()["rows"] == R and torch.equal(got, E.encode(module, ids))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_does_not_depend_on_its_neighbours(gpu_device, monkeypatch, dtype):
    from pww_hip import text_encode as E
    module = copy.deepcopy(tc.encoder("tiny", dtype)).to(gpu_device)
    ids, _ = tc.encoder_case("tiny", dtype, 3)
    monkeypatch.setenv("PWW_TEXT_LINEAR", "force")
    E.reset_stats()
    three = E.encode(module, ids)
    assert E.stats()["linear"]["stock"] == 0                                    # the all-native route
    for r in range(3):
        assert torch.equal(three[r:r + 1], E.encode(module, ids[r:r + 1])), r


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_cached_packed_weight_follows_the_module(gpu_device, dtype):
    from pww_hip import text_encode as E
    module = copy.deepcopy(tc.encoder("tiny", dtype)).to(gpu_device)
    ids, _ = tc.encoder_case("tiny", dtype, 1)
    before = E.encode(module, ids)
    a = module.encoder.layers[0].self_attn
    assert a.__dict__["_pww_text_qkv"][1].shape == (3 * 128, 128)
    a.q_proj.weight.mul_(-1.5)                                                  # in place: same storage, a new version
    after = E.encode(module, ids)
    assert not torch.equal(before, after)
    with torch.no_grad():
        stock = module(ids.to(gpu_device))[0]
    tc.check(after, stock, tc.reference(module, ids), "encode tiny %s after q_proj.weight changed" % dtype)
    a.k_proj.bias = torch.nn.Parameter(torch.zeros_like(a.k_proj.bias), requires_grad=False)       # replaced: another storage
    again = E.encode(module, ids)
    with torch.no_grad():
        stock = module(ids.to(gpu_device))[0]
    tc.check(again, stock, tc.reference(module, ids), "encode tiny %s after k_proj.bias was replaced" % dtype)


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_a_whole_request_encodes_in_two_calls(gpu_device, monkeypatch):
    from PIL import Image
    import paint_with_words as pw
    from pww_hip import text_encode as E
    from sd_standin import CLIPTextEncoder
    from gpu_util import uninstall_all
    dtype = torch.float16
    vae, unet, tiny_text, tok, sch = cases.build_tools("tiny", dtype=dtype, device=gpu_device)
    ctx_dim = tiny_text.pos.shape[1]                                            # the UNet's cross_attention_dim
    assert ctx_dim == 64
    clip = CLIPTextEncoder(ctx_dim=ctx_dim, layers=2, heads=1, intermediate=128, seed=9).to(device=gpu_device, dtype=dtype)
    prompt = cases.RUNNER_PROMPT + ", " + " ".join("detail%d" % i for i in range(90))      # two chunks
    colors = list(cases.RUNNER_CONTEXT)
    regions = {colors[0]: "an old oak tree with autumn leaves", colors[1]: "a white fluffy dog, studio photo"}

    def run(text):
        return pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(cases.load_example_rgb()), input_prompt=prompt,
                                   num_inference_steps=3, guidance_scale=7.5, seed=3, device=str(gpu_device), weight_function=cases.weight_fn_runner,
                                   preloaded_utils=(vae, unet, text, tok, sch), return_latents=True, region_prompts=dict(regions), max_prompt_chunks=2).clone()
    try:
        E.reset_stats()
        native = run(clip)
        st = E.stats()
        assert st["encodes"] == 2 and st["rows"] == 4 + 4, st                   # cond + uncond of two chunks; two regions of two chunks
        monkeypatch.setenv("PWW_TEXT_ENCODE", "0")
        E.reset_stats()
        stock = run(clip)
        assert E.stats()["encodes"] == 0
        monkeypatch.delenv("PWW_TEXT_ENCODE")
        err = _rel_l2(native, stock)
        print("whole request, native text encode against PWW_TEXT_ENCODE=0: rel-L2 %.3e" % err)
        assert torch.isfinite(native).all() and err <= 2e-2, err
        E.reset_stats()
        run(tiny_text)
        assert E.stats()["encodes"] == 0 and E.stats()["rows"] == 0           # an encoder the route does not cover never enters it
    finally:
        uninstall_all()
