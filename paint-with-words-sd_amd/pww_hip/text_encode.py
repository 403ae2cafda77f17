"""CLIP text encoder on the native path: token ids -> the last hidden state.

`encode(text_encoder, ids)` stands in for `text_encoder(ids)[0]` -- the hidden state after final_layer_norm, no attention mask, positions
0 .. L - 1, causal -- for a float16 / bfloat16 module with the CLIPTextModel layout (`covers(text_encoder)`: transformers 4.x keeps the model
under `.text_model`, 5.x on the module itself; sd_standin.CLIPTextEncoder has the 5.x form). Every row of a request goes through ONE forward
(conditioning.encode_rows), and a layer is eight launches instead of the stock module's fifteen or so:

  1. the packed q | k | v projection + bias: one GEMM on the concatenated [3 C, C] weight (cached per layer, `_qkv_weight`)
  2. the causal attention (pww_text_attn_fwd): reads the packed projection where it lies, writes the heads merged
  3. out_proj + bias
  4. ops.add_layer_norm(a=residual): the residual sum and layer_norm2 of it
  5. fc1 + bias
  6. QuickGELU / GELU in place (pww_text_act)
  7. fc2 + bias + residual: in the GEMM's epilogue on ops.linear; on the stock GEMM the add is folded into the launch of 8
  8. the next layer's layer_norm1, or final_layer_norm (ops.add_layer_norm)
The embedding gather, the position add and layer 0's layer_norm1 are one launch in front (pww_text_embed_ln).

GEMMs: each runs on ops.linear or on the stock GEMM by a MEASURED table keyed by (K, N) (`LINEAR_ROUTES`; profiles/text_encoder.md). The tile width
and K split handed to ops.linear depend on (K, N) alone, never on the row count, and neither do the other kernels: with every GEMM on
ops.linear (PWW_TEXT_LINEAR=force) a prompt's embedding is the same bits whether it is encoded alone or beside other rows.

Switches (environment, read per call): PWW_TEXT_ENCODE=0 keeps the stock module everywhere (`enabled()`); PWW_TEXT_EMBED=0 / PWW_TEXT_ATTN=0 /
PWW_TEXT_ACT=0 run that part as stock ops (PWW_TEXT_ACT=1 also runs GELU native: it measured slower than F.gelu and is off by default);
PWW_TEXT_LINEAR=0 keeps every GEMM stock, =force sends every GEMM ops.linear takes to it. Wherever a `*_takes` says no, that op runs as the
stock op and is counted (`stats()`). Defaults and the measurements behind them: profiles/text_encoder.md.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from ._lib import PwwHipError
from .ops import _DT, _ptr, _stream

_PARTS = ("embed", "attention", "act", "linear", "layer_norm")
_STATS = {k: [0, 0] for k in _PARTS}
_CALLS = [0, 0]         # encodes, rows
HEAD_DIM, MAX_TOKENS, MAX_WIDTH = _lib.TEXT_HEAD_DIM, _lib.TEXT_MAX_TOKENS, _lib.TEXT_MAX_WIDTH
LN_MAX_WIDTH = 2048     # ops.add_layer_norm: one wave per row, C <= 2048; a wider model keeps the stock route (covers)
ACTS = {"quick_gelu": _lib.TEXT_ACT_QUICK_GELU, "gelu": _lib.TEXT_ACT_GELU}

# (K, N) -> (tile_n, splitk) of the GEMMs that measured faster on ops.linear than on the stock GEMM at the row counts of a request (M = 154 and
# M = 1078), bf16 on MI355X: tools/time_text_encode.py, profiles/text_encoder.md section 3. A shape that is not here keeps the stock GEMM.
# EMPTY: at both topologies the stock GEMM won every shape at M = 154 -- 17.9 - 18.2 us against 18.6 - 19.0 for q | k | v, out_proj and fc1,
# 21.8 / 21.9 against 22.8 / 24.1 for fc2 + residual -- and ops.linear won a single cell, fc2 of SD2.x at M = 1078 (25.4 against 29.6), which a
# key of (K, N) alone cannot route without losing the plain request. The whole encode agrees: 2.41 ms with every GEMM stock, 2.87 ms with every
# GEMM forced (SD1.5, R = 2).
LINEAR_ROUTES = {}


def _gemm_plan(K, N):
    """(tile_n, splitk) ops.linear is given for a [N, K] weight (PWW_TEXT_LINEAR=force, or a row of the table): the table's, else the best of
    the sweep by K alone -- 64-wide tiles, unsplit up to K = 1024 (18.6 - 19.0 us; every split costs its fold launch: 22.3+), three splits
    from K = 2048 on (fc2: 23.9 - 25.7 us at both row counts; unsplit 22.8 - 32.4). Never a function of the row count."""
    hit = LINEAR_ROUTES.get((K, N))
    if hit is not None:
        return hit
    return 64, (3 if K >= 2048 else 1)


def enabled():
    """Default ON: measured, bf16, the native encode of a plain request (R = 2) on the SD1.5 topology takes 2.54 ms against 6.36 ms for the two
    stock calls of one row each; 2.62 ms against 45.4 ms at R = 14. SD2.x: 4.35 against 11.2 ms, 4.50 against 77.8 ms (profiles/text_encoder.md)."""
    return os.environ.get("PWW_TEXT_ENCODE", "1") != "0"


def embed_enabled():
    """Default ON: 14.9 us for the one launch against 16.9 us for embedding + add + layer_norm (R = 2, C 768; 14.5 / 16.7 at R = 14)."""
    return os.environ.get("PWW_TEXT_EMBED", "1") != "0"


def attn_enabled():
    """Default ON: 13.9 us at R = 2 (SD1.5) against 14.1 us for F.scaled_dot_product_attention(is_causal=True) + the merge -- a tie inside the
    spread of 6.6 % -- and 98.2 us for the eager sequence the module itself runs; 13.5 against 23.3 / 95.6 us at R = 14."""
    return os.environ.get("PWW_TEXT_ATTN", "1") != "0"


def act_enabled(act="quick_gelu"):
    """PWW_TEXT_ACT=1 / 0: on / off for both functions. Default: ON for quick_gelu -- 11.4 us against 12.3 us for the three launches of
    x * sigmoid(1.702 x) -- and OFF for gelu: F.gelu is ONE stock launch of 4.0 - 5.0 us, and pww_text_act's 10.9 us (the cost of a launch
    through this package, which every kernel here pays) is slower than it."""
    v = os.environ.get("PWW_TEXT_ACT")
    return v != "0" if v is not None else act == "quick_gelu"


def linear_mode():
    """"table" (default: LINEAR_ROUTES decides per shape), "0" (every GEMM stock) or "force" (every GEMM ops.linear takes)."""
    v = os.environ.get("PWW_TEXT_LINEAR", "table")
    return v if v in ("0", "force") else "table"


def stats():
    """{part: {"native": n, "stock": n}} since the last reset_stats(), "encodes": the calls of `encode`, "rows": the prompt rows they encoded.
    Parts: embed (gather + add + layer 0's layer_norm1), attention, act, linear (every GEMM), layer_norm (every other LayerNorm)."""
    out = {k: {"native": v[0], "stock": v[1]} for k, v in _STATS.items()}
    out["encodes"], out["rows"] = _CALLS
    return out


def reset_stats():
    for v in _STATS.values():
        v[0] = v[1] = 0
    _CALLS[0] = _CALLS[1] = 0


def _count(part, native):
    _STATS[part][0 if native else 1] += 1
    return native


# ---- the structural check ------------------------------------------------------------------------------------------------------------------
def _root(text_encoder):
    return getattr(text_encoder, "text_model", text_encoder)


def _is_linear(m, cin, cout):
    return type(m) is nn.Linear and m.bias is not None and m.in_features == cin and m.out_features == cout


def _is_ln(m, C):
    return isinstance(m, nn.LayerNorm) and tuple(m.normalized_shape) == (C,) and m.weight is not None and m.bias is not None


def covers(text_encoder, require_device=True):
    """True for a float16 / bfloat16 module on one HIP device with the CLIPTextModel layout, under `.text_model` (transformers 4.x) or on the
    module itself (5.x): embeddings.token_embedding / .position_embedding (nn.Embedding), encoder.layers[i] with .layer_norm1,
    .self_attn.{q,k,v,out}_proj (biased, C -> C), .layer_norm2, .mlp.fc1 / .fc2 (biased), final_layer_norm; config.num_attention_heads with
    C / heads == 64 and C <= 2048, config.hidden_act "quick_gelu" or "gelu", config.layer_norm_eps. TinyTextEncoder, an fp32 module, one on the CPU, another
    head dim, another activation or a projection without a bias is not covered. require_device=False: the layout and dtype checks alone."""
    try:
        root = _root(text_encoder)
        cfg = getattr(text_encoder, "config", None) or root.config
        emb = root.embeddings
        tok, pos = emb.token_embedding, emb.position_embedding
        if not (isinstance(tok, nn.Embedding) and isinstance(pos, nn.Embedding)):
            return False
        w = tok.weight
        C = w.shape[1]
        heads = int(cfg.num_attention_heads)
        if not (w.dtype in _DT and (w.is_cuda or not require_device) and pos.weight.shape[1] == C and C % 64 == 0 and C <= min(MAX_WIDTH, LN_MAX_WIDTH) and heads >= 1
                and C == heads * HEAD_DIM and cfg.hidden_act in ACTS and float(cfg.layer_norm_eps) > 0):
            return False
        if any(p.dtype != w.dtype or p.device != w.device for p in root.parameters()):
            return False
        layers = list(root.encoder.layers)
        if not layers or not _is_ln(root.final_layer_norm, C):
            return False
        inner = layers[0].mlp.fc1.out_features
        for layer in layers:
            a = layer.self_attn
            if not (_is_ln(layer.layer_norm1, C) and _is_ln(layer.layer_norm2, C) and all(_is_linear(m, C, C) for m in (a.q_proj, a.k_proj, a.v_proj, a.out_proj))
                    and _is_linear(layer.mlp.fc1, C, inner) and _is_linear(layer.mlp.fc2, inner, C) and inner % 8 == 0):
                return False
        return True
    except (AttributeError, TypeError, ValueError):
        return False


# ---- the three kernels of libpww_hip_text.so -----------------------------------------------------------------------------------------------
def embed_takes(ids, tok, pos, weight, bias):
    """True when pww_text_embed_ln runs this call: int32 [R, L] ids on a HIP device, float16 / bfloat16 tables [V, C] and [P, C] of one dtype on
    it with C a multiple of 64 (<= 4096) and L <= P, and a contiguous [C] affine of that dtype."""
    if not (torch.is_tensor(ids) and ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 2 and ids.numel() > 0 and torch.is_tensor(tok) and tok.dtype in _DT):
        return False
    C = tok.shape[-1]
    return (tok.dim() == 2 and pos.dim() == 2 and pos.shape[1] == C and C % 64 == 0 and C <= MAX_WIDTH and ids.shape[1] <= pos.shape[0]
            and all(t.dtype == tok.dtype and t.device == ids.device and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (tok, pos, weight, bias))
            and tuple(weight.shape) == (C,) and tuple(bias.shape) == (C,) and ids.numel() * C < 2 ** 31)


def embed_ln(ids, tok, pos, weight, bias, eps):
    """(x, h): x = tok[ids] + pos[:L] rounded as the stock add rounds it, h = LayerNorm(x) with fp32 statistics; [R, L, C] each, one launch.
    The caller has checked 0 <= id < V (the kernel clamps, it does not report)."""
    if not embed_takes(ids, tok, pos, weight, bias):
        raise PwwHipError("text_encode.embed_ln: needs int32 [R, L] ids on a HIP device, float16/bfloat16 [V, C] / [P, C] tables with C a multiple of 64, L <= P, "
                          "and a [C] affine of their dtype")
    ids = ids.contiguous()
    R, L = ids.shape
    C = tok.shape[1]
    x = torch.empty((R, L, C), dtype=tok.dtype, device=ids.device)
    h = torch.empty_like(x)
    lib = _lib.load_text()
    with torch.cuda.device(ids.device):
        _lib.check(lib.pww_text_embed_ln(_ptr(ids), _ptr(tok), _ptr(pos), _ptr(weight), _ptr(bias), _ptr(x), _ptr(h), R, L, C, tok.shape[0], pos.shape[0],
                                         float(eps), _DT[tok.dtype], _stream()), "pww_text_embed_ln", lib)
    return x, h


def embed_ln_stock(ids, tok, pos, weight, bias, eps):
    """The sequence the kernel replaces: the gather, the add, the LayerNorm."""
    x = F.embedding(ids.long(), tok) + pos[: ids.shape[1]]
    return x, F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def attn_takes(qkv, heads):
    """True when pww_text_attn_fwd runs this call: a float16 / bfloat16 [R, L, 3 C] (or [R L, 3 C] with rows=...) packed projection on a HIP
    device, C = 64 heads, 1 <= L <= 128, unit stride along the columns, one row pitch that is a multiple of 8 elements, 16-byte aligned."""
    if not (torch.is_tensor(qkv) and qkv.is_cuda and qkv.dtype in _DT and qkv.dim() == 3 and qkv.numel() > 0):
        return False
    R, L, C3 = qkv.shape
    r = ops._rows(qkv, "text_attn")
    return (heads >= 1 and C3 == 3 * heads * HEAD_DIM and 1 <= L <= MAX_TOKENS and r is not None and r[2] >= C3 and R * heads <= 65535
            and R * L * r[2] < 2 ** 31)


def attention(qkv, heads):
    """Causal self-attention of a packed [R, L, 3 C] projection (q | k | v, head h at columns 64 h of each) -> the dense [R, L, C] output with the
    heads merged. Scale 64^-0.5; fp32 scores and softmax, the normalised probabilities rounded to the storage type in front of P V."""
    if not attn_takes(qkv, heads):
        raise PwwHipError("text_encode.attention: needs a float16/bfloat16 [R, L, 3 * 64 * heads] tensor on a HIP device with one row pitch, 1 <= L <= 128")
    R, L, C3 = qkv.shape
    ld = ops._rows(qkv, "text_attn")[2]
    o = torch.empty((R, L, C3 // 3), dtype=qkv.dtype, device=qkv.device)
    lib = _lib.load_text()
    with torch.cuda.device(qkv.device):
        _lib.check(lib.pww_text_attn_fwd(_ptr(qkv), _ptr(o), R, heads, L, ld, C3 // 3, _DT[qkv.dtype], _stream()), "pww_text_attn_fwd", lib)
    return o


def attention_stock(qkv, heads):
    """The sequence the kernel replaces (transformers' eager CLIP attention): q k^T in the storage type, the scale, the causal mask, the softmax
    in fp32 cast back, the second product, the merge."""
    R, L, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(R, L, heads, C // heads).transpose(1, 2) for i in range(3))
    w = torch.matmul(q, k.transpose(-1, -2)) * (C // heads) ** -0.5
    w = w + torch.full((L, L), float("-inf"), dtype=w.dtype, device=w.device).triu(1)
    w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    return torch.matmul(w, v).transpose(1, 2).reshape(R, L, C)


def act_takes(x, act):
    """True when pww_text_act runs this call: a float16 / bfloat16 [..., N] tensor on a HIP device whose rows have one pitch (a multiple of 8
    elements, 16-byte aligned), N a multiple of 8, act "quick_gelu" or "gelu"."""
    if not (act in ACTS and torch.is_tensor(x) and x.is_cuda and x.dtype in _DT and x.dim() >= 2 and x.numel() > 0 and x.shape[-1] % 8 == 0):
        return False
    r = ops._rows(x, "text_act")
    return r is not None and r[0] * r[2] < 2 ** 31


def act_(x, act):
    """QuickGELU (x sigmoid(1.702 x)) or GELU (erf form) of x IN PLACE, fp32 with one rounding; returns x."""
    if not act_takes(x, act):
        raise PwwHipError("text_encode.act_: needs a float16/bfloat16 [..., N] tensor on a HIP device with one row pitch, N a multiple of 8, act quick_gelu / gelu")
    rows, N, stride = ops._rows(x, "text_act")
    lib = _lib.load_text()
    with torch.cuda.device(x.device):
        _lib.check(lib.pww_text_act(_ptr(x), rows, N, stride, ACTS[act], _DT[x.dtype], _stream()), "pww_text_act", lib)
    return x


def act_stock(x, act):
    """The expression the kernel replaces."""
    return x * torch.sigmoid(1.702 * x) if act == "quick_gelu" else F.gelu(x)


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------
def _qkv_weight(a):
    """The [3 C, C] weight and [3 C] bias of q | k | v, cached on the attention module and rebuilt when a parameter was replaced, modified in
    place, moved or cast (as vae._qkv_weight)."""
    params = [p for m in (a.q_proj, a.k_proj, a.v_proj) for p in (m.weight, m.bias)]
    key = tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in params)
    hit = a.__dict__.get("_pww_text_qkv")
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    w = torch.cat([a.q_proj.weight.detach(), a.k_proj.weight.detach(), a.v_proj.weight.detach()], 0).contiguous()
    b = torch.cat([a.q_proj.bias.detach(), a.k_proj.bias.detach(), a.v_proj.bias.detach()], 0).contiguous()
    a.__dict__["_pww_text_qkv"] = (key, w, b)
    return w, b


def _linear(x, weight, bias, mode, residual=None):
    """x weight^T + bias (+ residual) on ops.linear where the route says so; -> (y, whether the residual is in y)."""
    N, K = weight.shape
    native = mode != "0" and (mode == "force" or (K, N) in LINEAR_ROUTES) and ops.linear_takes(x, weight, bias=bias, residual=residual)
    if _count("linear", native):
        tile_n, splitk = _gemm_plan(K, N)
        return ops.linear(x, weight, bias, residual=residual, tile_n=tile_n, splitk=splitk), True
    return F.linear(x, weight, bias), False


def _layer_norm(x, ln, a=None):
    _count("layer_norm", True)
    return ops.add_layer_norm(x, ln.weight, ln.bias, ln.eps, a=a)


def encode_stock(text_encoder, ids):
    """The route of before: one call of the module per row, a [1, L] batch each, concatenated."""
    return torch.cat([text_encoder(ids[r:r + 1])[0] for r in range(ids.shape[0])], 0)


def encode(text_encoder, ids):
    """`text_encoder(ids)[0]` for a module `covers()` accepts: ids [R, L] integers (CPU or device) -> [R, L, C] in the module's dtype, every row
    in one forward. Ids on the CPU (what a tokenizer returns) are checked against the vocabulary there; ids on the device are taken as given."""
    if not covers(text_encoder):
        raise PwwHipError("text_encode.encode: the module has not the CLIPTextModel layout in float16/bfloat16 on a HIP device (pww_hip.text_encode.covers)")
    if not (torch.is_tensor(ids) and ids.dim() == 2 and ids.numel() > 0 and not ids.is_floating_point() and ids.dtype != torch.bool):
        raise PwwHipError("text_encode.encode: ids must be a [R, L] integer tensor")
    root = _root(text_encoder)
    cfg = getattr(text_encoder, "config", None) or root.config
    tok, pos = root.embeddings.token_embedding.weight, root.embeddings.position_embedding.weight
    dev, heads, act = tok.device, int(cfg.num_attention_heads), cfg.hidden_act
    R, L = ids.shape
    if L > pos.shape[0]:
        raise PwwHipError("text_encode.encode: %d tokens exceed the %d positions of the model" % (L, pos.shape[0]))
    if not ids.is_cuda and (int(ids.min()) < 0 or int(ids.max()) >= tok.shape[0]):
        raise PwwHipError("text_encode.encode: token ids must be in [0, %d)" % tok.shape[0])
    ids = ids.to(device=dev, dtype=torch.int32)
    mode = linear_mode()
    layers = list(root.encoder.layers)
    _CALLS[0] += 1
    _CALLS[1] += R
    with torch.no_grad():
        ln = layers[0].layer_norm1
        if _count("embed", embed_enabled() and embed_takes(ids, tok, pos, ln.weight, ln.bias)):
            x, h = embed_ln(ids, tok, pos, ln.weight, ln.bias, ln.eps)
        else:
            x, h = embed_ln_stock(ids, tok, pos, ln.weight, ln.bias, ln.eps)
        for i, layer in enumerate(layers):
            a = layer.self_attn
            w, b = _qkv_weight(a)
            qkv, _ = _linear(h, w, b, mode)
            if _count("attention", attn_enabled() and attn_takes(qkv, heads)):
                o = attention(qkv, heads)
            else:
                o = attention_stock(qkv, heads)
            y, _ = _linear(o, a.out_proj.weight, a.out_proj.bias, mode)
            x, h = _layer_norm(y, layer.layer_norm2, a=x)
            f, _ = _linear(h, layer.mlp.fc1.weight, layer.mlp.fc1.bias, mode)
            if _count("act", act_enabled(act) and act_takes(f, act)):
                f = act_(f, act)
            else:
                f = act_stock(f, act)
            nxt = layers[i + 1].layer_norm1 if i + 1 < len(layers) else root.final_layer_norm
            y, summed = _linear(f, layer.mlp.fc2.weight, layer.mlp.fc2.bias, mode, residual=x)
            if summed:
                x, h = y, _layer_norm(y, nxt)
            else:
                x, h = _layer_norm(y, nxt, a=x)
    return h
