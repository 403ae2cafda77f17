"""Tokenizer / text-encoder stand-ins.

The reference uses the CLIP tokenizer and text model of the SD checkpoint
(paint_with_words/paint_with_words.py:170-171); neither vocabulary nor weights exist offline. The
hot path only needs (a) token ids framed BOS ... EOS and padded to 77 so that region phrases can be
matched against the prompt (:222-227, :251-260) and (b) a [1, 77, ctx_dim] embedding (:360-368).
"""
import re
import zlib
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

BOS, EOS = 49406, 49407


class _Encoding(dict):
    """Mapping with attribute access, like transformers' BatchEncoding (:251 uses ["input_ids"], :360 .input_ids)."""
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class HashTokenizer:
    """Deterministic word-level tokenizer: lower-cased words and punctuation marks hash to ids in
    [1000, 49000); BOS=49406, EOS=49407, padding with EOS (the CLIP conventions)."""
    model_max_length = 77

    _pat = re.compile(r"[a-z0-9]+|[^\sa-z0-9]", re.IGNORECASE)

    def _ids(self, text):
        return [1000 + zlib.crc32(w.lower().encode("utf-8")) % 48000 for w in self._pat.findall(text)]

    def __call__(self, text, padding=False, max_length=None, truncation=False, return_tensors=None):
        batched = isinstance(text, (list, tuple))
        texts = list(text) if batched else [text]
        max_length = max_length or self.model_max_length
        out = []
        for t in texts:
            ids = self._ids(t)
            if truncation or True:
                ids = ids[: max_length - 2]
            ids = [BOS] + ids + [EOS]
            if padding == "max_length":
                ids = ids + [EOS] * (max_length - len(ids))
            out.append(ids)
        if return_tensors == "pt":
            return _Encoding(input_ids=torch.tensor(out, dtype=torch.long))
        return _Encoding(input_ids=out if batched else out[0])


class TinyTextEncoder(nn.Module):
    """Random-init embedding + position + LayerNorm text encoder: returns ([B, 77, ctx_dim],)."""

    def __init__(self, ctx_dim=768, vocab=49408, max_len=77, seed=1235):
        super().__init__()
        state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        try:
            self.tok = nn.Embedding(vocab, ctx_dim)
            self.pos = nn.Parameter(torch.randn(max_len, ctx_dim) * 0.1)
            self.norm = nn.LayerNorm(ctx_dim)
        finally:
            torch.random.set_rng_state(state)
        self.requires_grad_(False)

    @property
    def dtype(self):
        return self.pos.dtype

    def forward(self, input_ids):
        x = self.tok(input_ids) + self.pos[: input_ids.shape[1]]
        return (self.norm(x),)


class _ClipEmbeddings(nn.Module):
    def __init__(self, vocab, max_len, dim):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, dim)
        self.position_embedding = nn.Embedding(max_len, dim)

    def forward(self, input_ids):
        return self.token_embedding(input_ids) + self.position_embedding.weight[: input_ids.shape[1]]


class _ClipAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.num_heads, self.head_dim, self.scale = heads, dim // heads, (dim // heads) ** -0.5
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(dim, dim) for _ in range(4))

    def forward(self, x):
        """The eager attention of transformers' CLIP: scores and output as products in x's dtype, the causal mask added, the softmax of a
        float16 / bfloat16 tensor in fp32 and cast back in front of the second product (fp32 and fp64 keep their own precision)."""
        B, L, C = x.shape
        q, k, v = (p(x).view(B, L, self.num_heads, self.head_dim).transpose(1, 2) for p in (self.q_proj, self.k_proj, self.v_proj))
        w = torch.matmul(q, k.transpose(-1, -2)) * self.scale
        w = w + torch.full((L, L), float("-inf"), dtype=w.dtype, device=w.device).triu(1)
        w = F.softmax(w, dim=-1, dtype=torch.float32 if w.dtype in (torch.float16, torch.bfloat16) else None).to(q.dtype)
        return self.out_proj(torch.matmul(w, v).transpose(1, 2).reshape(B, L, C))


class _ClipMLP(nn.Module):
    def __init__(self, dim, intermediate, hidden_act):
        super().__init__()
        self.hidden_act = hidden_act
        self.fc1, self.fc2 = nn.Linear(dim, intermediate), nn.Linear(intermediate, dim)

    def forward(self, x):
        x = self.fc1(x)
        return self.fc2(x * torch.sigmoid(1.702 * x) if self.hidden_act == "quick_gelu" else F.gelu(x))


class _ClipLayer(nn.Module):
    def __init__(self, dim, heads, intermediate, hidden_act, eps):
        super().__init__()
        self.self_attn = _ClipAttention(dim, heads)
        self.layer_norm1 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _ClipMLP(dim, intermediate, hidden_act)
        self.layer_norm2 = nn.LayerNorm(dim, eps=eps)

    def forward(self, x):
        x = x + self.self_attn(self.layer_norm1(x))
        return x + self.mlp(self.layer_norm2(x))


class _ClipEncoder(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.ModuleList(layers)


class CLIPTextEncoder(nn.Module):
    """Random-init CLIP text model in plain torch with the attribute layout of transformers 5.x's CLIPTextModel (`embeddings`, `encoder.layers`
    and `final_layer_norm` on the model itself; 4.x keeps the same three under `.text_model`) and its state-dict keys, and a small `config`
    namespace. forward(input_ids) -> (last_hidden_state,): no attention mask, positions 0 .. L - 1, causal. hidden_act: "quick_gelu" (SD1.x)
    or "gelu" (SD2.x)."""

    def __init__(self, ctx_dim=768, layers=12, heads=12, intermediate=3072, hidden_act="quick_gelu", vocab=49408, max_len=77, seed=1235):
        super().__init__()
        if hidden_act not in ("quick_gelu", "gelu") or ctx_dim % heads:
            raise ValueError("CLIPTextEncoder: hidden_act must be 'quick_gelu' or 'gelu' and heads must divide ctx_dim")
        self.config = SimpleNamespace(hidden_size=ctx_dim, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=intermediate,
                                      hidden_act=hidden_act, layer_norm_eps=1e-5, vocab_size=vocab, max_position_embeddings=max_len)
        state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        try:
            self.embeddings = _ClipEmbeddings(vocab, max_len, ctx_dim)
            self.encoder = _ClipEncoder([_ClipLayer(ctx_dim, heads, intermediate, hidden_act, 1e-5) for _ in range(layers)])
            self.final_layer_norm = nn.LayerNorm(ctx_dim, eps=1e-5)
            # (the defaults of nn.Linear leave the biases and the norms' affines near their identities: give them some size, so that a kernel
            # that drops one of them fails its test)
            for name, p in self.named_parameters():
                if name.endswith(".bias"):
                    p.data.normal_(0.0, 0.05)
                elif "layer_norm" in name:
                    p.data.add_(torch.randn_like(p) * 0.05)
        finally:
            torch.random.set_rng_state(state)
        self.requires_grad_(False)

    @property
    def dtype(self):
        return self.final_layer_norm.weight.dtype

    def forward(self, input_ids):
        x = self.embeddings(input_ids)
        for layer in self.encoder.layers:
            x = layer(x)
        return (self.final_layer_norm(x),)


def build_clip_text_encoder(ctx_dim=768, seed=1235, device="cpu", dtype=torch.float32):
    """Random-init transformers CLIPTextModel with SD1.x (ctx_dim 768) / SD2.x (1024) sizes; falls back to
    TinyTextEncoder if transformers cannot build it offline."""
    try:
        from transformers import CLIPTextConfig, CLIPTextModel
        layers, heads, inter = (12, 12, 3072) if ctx_dim == 768 else (23, 16, 4096)
        cfg = CLIPTextConfig(vocab_size=49408, hidden_size=ctx_dim, intermediate_size=inter, num_hidden_layers=layers,
                             num_attention_heads=heads, max_position_embeddings=77)
        state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        try:
            enc = CLIPTextModel(cfg)
        finally:
            torch.random.set_rng_state(state)
        return enc.to(device=device, dtype=dtype).eval().requires_grad_(False)
    except Exception:
        return TinyTextEncoder(ctx_dim, seed=seed).to(device=device, dtype=dtype).eval()
