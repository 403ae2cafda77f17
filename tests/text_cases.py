"""Inputs, the reference and the bar of the CLIP text encoder tests (test_text_host.py, test_text_kernels_gpu.py, test_text_encode_gpu.py).

The reference is a restatement of the CLIP text forward on the module's state dict upcast to fp64, written out plainly. The rule of every
comparison is the project's (test_attention_gpu.py, vae_cases.py):

    err(native vs reference) <= 1.5 * err(stock same-dtype op sequence vs reference) + 2e-3 * max|reference|

with the stock error measured per case on the same inputs, never against the code under test.
"""
import functools

import torch
import torch.nn.functional as F

BOS, EOS = 49406, 49407
TOPOLOGIES = {
    "tiny": dict(ctx_dim=128, heads=2, layers=2, intermediate=256, hidden_act="quick_gelu"),
    "sd15": dict(ctx_dim=768, heads=12, layers=2, intermediate=3072, hidden_act="quick_gelu"),
    "sd2": dict(ctx_dim=1024, heads=16, layers=1, intermediate=4096, hidden_act="gelu"),
}


def bar(stock, ref):
    ref = ref.double().cpu()
    return 1.5 * (stock.double().cpu() - ref).abs().max().item() + 2e-3 * ref.abs().max().item()


def check(native, stock, ref, what):
    """One comparison under the rule above; prints the figures before it asserts. Returns the bar."""
    eps = bar(stock, ref)
    err = (native.double().cpu() - ref.double().cpu()).abs().max().item()
    peak = ref.abs().max().item()
    print("%s: err %.3e, bar %.3e (stock err %.3e, max|ref| %.3e)" % (what, err, eps, (eps - 2e-3 * peak) / 1.5, peak))
    assert tuple(native.shape) == tuple(ref.shape), (what, native.shape, ref.shape)
    assert torch.isfinite(native.float()).all(), what
    assert err <= eps, (what, err, eps)
    return eps


def prompt_ids(R, L=77, vocab=49408, seed=0):
    """[R, L] int64 ids framed BOS ... EOS and padded with EOS, as the tokenizer frames them; row r carries 3 + 11 r content tokens (capped).
    For a vocabulary below 49408 the frame ids are vocab - 2 and vocab - 1."""
    bos, eos = (BOS, EOS) if vocab > EOS else (vocab - 2, vocab - 1)
    g = torch.Generator().manual_seed(100 + seed)
    rows = []
    for r in range(R):
        n = min(max(L - 2, 0), 3 + 11 * r)
        body = torch.randint(0, bos, (n,), generator=g).tolist()
        rows.append(([bos] + body + [eos] * L)[:L])
    return torch.tensor(rows, dtype=torch.long)


def _root_state(module):
    return {k[len("text_model."):] if k.startswith("text_model.") else k: v for k, v in module.state_dict().items()}


def reference(module, ids):
    """The CLIP text forward restated on the module's state dict in fp64 (CPU): embeddings, then per layer x += out(attn(LN1(x))) with
    softmax(q k^T d^-0.5 + triu(-inf, 1)), x += fc2(act(fc1(LN2(x)))), then the final LayerNorm. -> [R, L, C] fp64."""
    sd = {k: v.detach().double().cpu() for k, v in _root_state(module).items()}
    cfg = module.config
    heads, act, eps = int(cfg.num_attention_heads), cfg.hidden_act, float(cfg.layer_norm_eps)
    ids = ids.cpu().long()
    R, L = ids.shape
    x = sd["embeddings.token_embedding.weight"][ids] + sd["embeddings.position_embedding.weight"][:L]
    C = x.shape[-1]
    d = C // heads
    mask = torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)

    def ln(t, name):
        return F.layer_norm(t, (C,), sd[name + ".weight"], sd[name + ".bias"], eps)

    def lin(t, name):
        return t @ sd[name + ".weight"].T + sd[name + ".bias"]
    i = 0
    while "encoder.layers.%d.layer_norm1.weight" % i in sd:
        p = "encoder.layers.%d." % i
        h = ln(x, p + "layer_norm1")
        q, k, v = (lin(h, p + "self_attn.%s_proj" % n).reshape(R, L, heads, d).transpose(1, 2) for n in "qkv")
        w = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1)
        x = x + lin((w @ v).transpose(1, 2).reshape(R, L, C), p + "self_attn.out_proj")
        f = lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")
        f = f * torch.sigmoid(1.702 * f) if act == "quick_gelu" else 0.5 * f * (1.0 + torch.erf(f / 2.0 ** 0.5))
        x = x + lin(f, p + "mlp.fc2")
        i += 1
    return ln(x, "final_layer_norm")


@functools.lru_cache(maxsize=None)
def encoder(name, dtype, vocab=1000):
    """The stand-in of TOPOLOGIES[name] in `dtype` on the CPU (vocabulary 1000: the table is the slow part of building one). Shared: do not modify."""
    from sd_standin import CLIPTextEncoder
    return CLIPTextEncoder(vocab=vocab, seed=7, **TOPOLOGIES[name]).to(dtype).eval()


@functools.lru_cache(maxsize=None)
def encoder_case(name, dtype, R, L=77):
    """(ids [R, L], reference [R, L, C] fp64) for encoder(name, dtype): the reference of the ROUNDED weights. Shared: do not modify."""
    ids = prompt_ids(R, L, vocab=1000, seed=R)
    return ids, reference(encoder(name, dtype), ids)


# ---- kernel inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def qkv_case(R, H, L, dtype, hot=False, seed=0):
    """A packed projection [R, L, 3 * 64 H] in `dtype` (CPU) and its fp64 causal attention [R, L, 64 H]. hot: q and k scaled so that the scaled
    logits q . k / 8 have a standard deviation of 8 (unit q, k give 1)."""
    g = torch.Generator().manual_seed(1000 * R + 10 * H + L + seed)
    C = 64 * H
    qkv = torch.randn(R, L, 3 * C, generator=g)
    if hot:
        qkv[..., :2 * C] *= 8.0 ** 0.5
    qkv = qkv.to(dtype)
    return qkv, attention_reference(qkv, H)


def attention_reference(qkv, H):
    R, L, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (qkv.double().cpu()[..., i * C:(i + 1) * C].reshape(R, L, H, 64).transpose(1, 2) for i in range(3))
    w = torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5 + torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1), dim=-1)
    return (w @ v).transpose(1, 2).reshape(R, L, C)


def act_reference(x, act):
    x = x.double()
    return x * torch.sigmoid(1.702 * x) if act == "quick_gelu" else 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))
