"""Host-side checks of the attention-map recording mode (pww_hip.record_attention_maps): the C ABI of pww_cross_attn_probs without a
device (validation precedes the first HIP call), AttentionMaps on hand-made tensors, the recorder's life cycle."""
import ctypes
import os
import re

import pytest
import torch

import pww_cases as cases  # noqa: F401  (puts the package on sys.path)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(L, N=64, M=77, D=40, H=8, dtype=0):
    d = L.AttnDesc()
    d.dtype, d.B, d.H, d.N, d.M, d.D = dtype, 2, H, N, M, D
    d.q_stride[:] = [N * H * D, D, H * D]
    d.k_stride[:] = [M * H * D, D, H * D]
    d.scale = D ** -0.5
    d.bias_stride[:] = [0, 0, M, 1]
    return d


def _pdesc(L, M=77, size=None):
    pd = L.ProbsDesc(ctypes.sizeof(L.ProbsDesc) if size is None else size, 0, 0, 1.0)
    pd.out_stride[:] = [64 * 80, (M + 3) // 4 * 4]
    return pd


def _call(lib, L, d, pd, q=0x10000, k=0x20000, out=0x30000, stats=None, kind=0):
    vp = ctypes.c_void_p
    return lib.pww_cross_attn_probs(vp(q), vp(k), vp(0), vp(stats or 0), kind, 1.0, 1.0, vp(0), ctypes.byref(d), None, vp(out), ctypes.byref(pd), vp(0))


def test_probs_export_layout_and_validation_without_a_device():
    """The library exports pww_cross_attn_probs; the binding's struct has the header's layout; bad arguments are refused with the
    documented codes and a message BEFORE any HIP call (so this runs on a machine without a GPU)."""
    import pww_hip
    from pww_hip import _lib as L
    lib = L.load()
    assert "pww_cross_attn_probs" in L.EXPORTS and hasattr(lib, "pww_cross_attn_probs")
    assert lib.pww_version() == 127
    # uint32 size, int32 images, int32 accumulate, float weight, int64 out_stride[2]
    assert ctypes.sizeof(L.ProbsDesc) == 32
    assert (L.ProbsDesc.images.offset, L.ProbsDesc.accumulate.offset, L.ProbsDesc.weight.offset, L.ProbsDesc.out_stride.offset) == (4, 8, 12, 16)
    header = open(os.path.join(REPO, "include", "pww_hip.h")).read()
    body = header[header.index("typedef struct pww_probs_desc {"):header.index("} pww_probs_desc_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == ["size", "images", "accumulate", "weight", "out_stride"]
    assert header.index("pww_cross_attn_probs(") < header.index("= experiments =")      # a product entry point, not an experiment

    def err():
        return lib.pww_last_error().decode()

    for size in (0, ctypes.sizeof(L.ProbsDesc) - 8):
        assert _call(lib, L, _desc(L), _pdesc(L, size=size)) == L.PWW_EINVAL
        assert "size" in err()
    assert _call(lib, L, _desc(L, M=129), _pdesc(L, M=129)) == L.PWW_ENOTSUP and err()
    assert _call(lib, L, _desc(L, D=12), _pdesc(L)) == L.PWW_ENOTSUP and err()
    assert _call(lib, L, _desc(L, D=168), _pdesc(L)) == L.PWW_ENOTSUP
    assert _call(lib, L, _desc(L, dtype=7), _pdesc(L)) == L.PWW_ENOTSUP
    assert _call(lib, L, _desc(L), _pdesc(L), q=0) == L.PWW_EINVAL and err()
    assert _call(lib, L, _desc(L), _pdesc(L), out=0x30004) == L.PWW_EINVAL and "aligned" in err()
    assert _call(lib, L, _desc(L), _pdesc(L), kind=1) == L.PWW_EINVAL and "stats" in err()      # a statistic without its statistics
    assert _call(lib, L, _desc(L), _pdesc(L), kind=6) == L.PWW_EINVAL                          # PWW_STAT_ALL selects nothing
    pd = _pdesc(L)
    pd.out_stride[1] = 77                                   # rows of 77 floats are not 16-byte aligned
    assert _call(lib, L, _desc(L), pd) == L.PWW_EINVAL and "stride" in err()
    pd = _pdesc(L)
    pd.out_stride[1] = 76                                   # shorter than M
    assert _call(lib, L, _desc(L), pd) == L.PWW_EINVAL
    pd = _pdesc(L)
    pd.images = 3                                           # more than B
    assert _call(lib, L, _desc(L), pd) == L.PWW_EINVAL
    d = _desc(L)
    d.q_stride[2] = 324                                     # not a multiple of 8
    assert _call(lib, L, d, _pdesc(L)) == L.PWW_EINVAL
    assert pww_hip.record_attention_maps is not None and pww_hip.AttentionMaps is not None


def _maps(per_layer=False):
    from pww_hip.attnmaps import AttentionMaps
    from sd_standin import HashTokenizer
    tok = HashTokenizer()
    prompt = "a photo of a dog and a cat"
    ids = tok([prompt], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")["input_ids"][0].tolist()
    M = len(ids)
    g = torch.Generator().manual_seed(0)
    a16 = torch.rand(2, 16, M, generator=g)                # one layer of 4 x 4 tokens, 3 contributions
    b16 = torch.rand(2, 16, M, generator=g)                # a second layer of 4 x 4 tokens, 1 contribution
    c4 = torch.rand(2, 4, M, generator=g)                  # one layer of 2 x 2 tokens, 2 contributions
    if per_layer:
        entries = [(16, a16 * 3, 3), (4, c4 * 2, 2), (16, b16 * 1, 1)]
    else:
        entries = [(16, a16 * 3 + b16, 4), (4, c4 * 2, 2)]
    return AttentionMaps(entries, latent_hw=(4, 4), tokenizer=tok, prompts=[ids]), (a16, b16, c4), ids, tok


def test_attention_maps_arithmetic():
    import torch.nn.functional as F
    maps, (a16, b16, c4), ids, tok = _maps()
    assert maps.resolutions == {16: (4, 4), 4: (2, 2)} and maps.counts == {16: 4, 4: 2}
    M = len(ids)
    mean16 = (a16 * 3 + b16) / 4
    torch.testing.assert_close(maps.raw(16), mean16.reshape(2, 4, 4, M))            # division by the contribution count
    torch.testing.assert_close(maps.raw(4), c4.reshape(2, 2, 2, M))
    up = F.interpolate(c4.reshape(2, 2, 2, M).permute(0, 3, 1, 2), size=(4, 4), mode="bilinear", align_corners=False)
    want = (mean16.reshape(2, 4, 4, M).permute(0, 3, 1, 2) * 4 + up * 2) / 6      # resolutions weighted by their layer counts
    torch.testing.assert_close(maps.tokens(), want)
    assert tuple(maps.tokens(size=(8, 8)).shape) == (2, M, 8, 8)
    # phrase -> prompt positions, the span search of conditioning._parse_regions / _column_lists
    dog = tok("dog", max_length=tok.model_max_length, truncation=True)["input_ids"][1:-1]
    col = ids.index(dog[0])
    assert maps.columns("dog") == [col]
    torch.testing.assert_close(maps.phrase("dog"), want[:, col])
    two = maps.columns("a dog")
    assert len(two) == 2 and two[1] == col
    torch.testing.assert_close(maps.phrase("a dog"), want[:, two].mean(1))
    import pww_hip
    with pytest.raises(pww_hip.PwwHipError):
        maps.columns("zebra")
    pil = maps.to_pil("cat", size=(8, 8))
    assert len(pil) == 2 and pil[0].size == (8, 8) and pil[0].mode == "L"
    lo, hi = pil[0].getextrema()
    assert (lo, hi) == (0, 255)                             # min-max normalised
    # per-layer maps: their count-weighted mean is the default map
    per, _, _, _ = _maps(per_layer=True)
    layers = per.layers
    assert len(layers) == 3 and [m.count for m in layers] == [3, 2, 1]
    mix = sum(m.tokens(size=(4, 4)) * m.count for m in layers) / sum(m.count for m in layers)
    torch.testing.assert_close(mix, want)
    torch.testing.assert_close(per.tokens(), want)


def test_recorder_life_cycle(monkeypatch):
    import pww_hip
    from pww_hip import attnmaps, attention, ops
    assert attnmaps.active() is None
    with pww_hip.record_attention_maps() as rec:
        assert attnmaps.active() is rec and rec.per_layer is False
        with pytest.raises(pww_hip.PwwHipError, match="nest"):
            with pww_hip.record_attention_maps():
                pass
        assert attnmaps.active() is rec                     # the refused inner block left the outer one alone
    assert attnmaps.active() is None
    with pytest.raises(ZeroDivisionError):
        with pww_hip.record_attention_maps(per_layer=True) as rec:
            assert rec.per_layer
            1 / 0
    assert attnmaps.active() is None                        # an exception inside the block leaves no recorder behind
    with pytest.raises(pww_hip.PwwHipError):
        rec.maps()                                          # nothing was recorded
    # a recorder on another thread does not show here
    import threading
    seen = []
    with pww_hip.record_attention_maps():
        t = threading.Thread(target=lambda: seen.append(attnmaps.active()))
        t.start()
        t.join()
    assert seen == [None]

    # the plug: a dict context WITHOUT the key never reaches attention_probs, and the sampler removes the key when a request ends
    class Stop(Exception):
        pass

    calls = []

    def fake_attention(q, k, v, heads, scale, **kw):
        calls.append(kw)
        raise Stop()

    def no_probs(*a, **kw):
        raise AssertionError("attention_probs called without a recorder in the context")

    monkeypatch.setattr(ops, "attention", fake_attention)
    monkeypatch.setattr(ops, "attention_probs", no_probs)
    monkeypatch.setattr(ops, "qk_parts", lambda *a, **kw: None)
    from sd_standin import CrossAttention
    mod = CrossAttention(64, 32, 2, 32).half()

    class FakeCuda(torch.Tensor):
        is_cuda = True

    hidden = torch.randn(1, 16, 64).half().as_subclass(FakeCuda)
    ctx = {"CONTEXT_TENSOR": torch.randn(1, 77, 32).half(), "CROSS_ATTENTION_WEIGHT_16": torch.rand(16, 77), "SIGMA": torch.tensor(3.0),
           "WEIGHT_FUNCTION": lambda w, sigma, qk: 0.3 * w * sigma}
    with pytest.raises(Stop):
        attention._attention(mod, hidden, ctx, None)
    assert len(calls) == 1 and calls[0].get("stats_out") is None
    assert attention.ATTN_RECORDER not in ctx


def test_recorder_refuses_a_process_group(monkeypatch):
    import pww_hip
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    with pytest.raises(pww_hip.PwwHipError, match="world size"):
        with pww_hip.record_attention_maps():
            pass
    from pww_hip import attnmaps
    assert attnmaps.active() is None
