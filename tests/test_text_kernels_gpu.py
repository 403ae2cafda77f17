"""The three kernels of libpww_hip_text.so against fp64, in fp16 and bf16, under the bar of text_cases.py: the stock torch op sequence in the
same dtype on the same inputs on the same GPU sets the allowance."""
import pytest
import torch
import torch.nn.functional as F

import text_cases as tc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


# ---- embed_ln ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,L,C", [(1, 1, 64), (2, 77, 64), (2, 77, 768), (3, 5, 1024)])
def test_embed_ln(gpu_device, dtype, R, L, C):
    from pww_hip import text_encode as E
    V, P = 1000, 77
    g = torch.Generator().manual_seed(R * 1000 + L + C)
    tok, pos = torch.randn(V, C, generator=g).to(dtype), (torch.randn(P, C, generator=g) * 0.1).to(dtype)
    w, b = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dtype), (0.1 * torch.randn(C, generator=g)).to(dtype)
    ids = torch.randint(0, V, (R, L), generator=g)
    ids.view(-1)[0] = 0
    ids.view(-1)[-1] = V - 1
    dev = [t.to(gpu_device) for t in (tok, pos, w, b)]
    x, h = E.embed_ln(ids.to(gpu_device, torch.int32), *dev, 1e-5)
    xs, hs = E.embed_ln_stock(ids.to(gpu_device), *dev, 1e-5)
    want = tok[ids] + pos[:L]                                                   # the add of two T tensors, on the CPU
    assert tuple(x.shape) == (R, L, C) and x.dtype == dtype and torch.equal(x.cpu(), want) and torch.equal(xs.cpu(), want)
    ref = F.layer_norm(want.double(), (C,), w.double(), b.double(), 1e-5)
    tc.check(h, hs, ref, "embed_ln %s R %d L %d C %d" % (dtype, R, L, C))
    x2, h2 = E.embed_ln(ids.to(gpu_device, torch.int32), *dev, 1e-5)
    assert torch.equal(x, x2) and torch.equal(h, h2)                            # bitwise repeatable


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(1, 1, 1), (1, 1, 32), (1, 2, 33), (2, 2, 64), (1, 1, 65), (3, 12, 77), (1, 16, 77), (1, 2, 128)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,H,L", ATTN_SHAPES)
def test_attention_parity_and_row_zero(gpu_device, dtype, R, H, L):
    from pww_hip import text_encode as E
    qkv, ref = tc.qkv_case(R, H, L, dtype)
    d = qkv.to(gpu_device)
    o = E.attention(d, H)
    tc.check(o, E.attention_stock(d, H), ref, "attention %s R %d H %d L %d" % (dtype, R, H, L))
    assert o.dtype == dtype and o.is_contiguous()
    assert torch.equal(o[:, 0].cpu(), qkv[:, 0, 2 * 64 * H:])                  # row 0 sees key 0 alone: v[0], bit for bit
    assert torch.equal(o, E.attention(d, H))                                    # bitwise repeatable


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_is_causal(gpu_device, dtype):
    from pww_hip import text_encode as E
    R, H, L = 2, 2, 77
    qkv, _ = tc.qkv_case(R, H, L, dtype)
    C = 64 * H
    base = E.attention(qkv.to(gpu_device), H).cpu()
    g = torch.Generator().manual_seed(5)
    for p in (1, 32, 33, 76):
        other = qkv.clone()
        other[:, p:, C:] = (3.0 * torch.randn(R, L - p, 2 * C, generator=g)).to(dtype)          # K and V at positions >= p
        got = E.attention(other.to(gpu_device), H).cpu()
        assert torch.equal(got[:, :p], base[:, :p]), p
        assert not torch.equal(got[:, p:], base[:, p:]), p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,H,L", [(1, 1, 1), (1, 2, 33), (3, 12, 77), (1, 2, 128)])
def test_attention_ragged_end(gpu_device, dtype, R, H, L):
    """The tensor is the first R L rows of a larger allocation that is NaN behind it: a key index past L must not be read from there."""
    from pww_hip import text_encode as E
    qkv, ref = tc.qkv_case(R, H, L, dtype)
    C3 = 3 * 64 * H
    big = torch.full((R * L + 64, C3), float("nan"), dtype=dtype, device=gpu_device)
    big[:R * L] = qkv.reshape(R * L, C3).to(gpu_device)
    view = big[:R * L].view(R, L, C3)
    o = E.attention(view, H)
    assert torch.isfinite(o.float()).all()
    assert torch.equal(o, E.attention(qkv.to(gpu_device), H))
    assert torch.isnan(big[R * L:].float()).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_hot_logits(gpu_device, dtype):
    from pww_hip import text_encode as E
    R, H, L = 2, 2, 77
    qkv, ref = tc.qkv_case(R, H, L, dtype, hot=True)
    C = 64 * H
    q, k = qkv[..., :64].double(), qkv[..., C:C + 64].double()
    std = (q @ k.transpose(-1, -2) / 8.0).std().item()
    assert 6.0 < std < 10.0, std                                                # the scaled logits have a standard deviation of about 8
    d = qkv.to(gpu_device)
    o = E.attention(d, H)
    tc.check(o, E.attention_stock(d, H), ref, "attention hot %s" % dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_strided_and_head_independent(gpu_device, dtype):
    from pww_hip import text_encode as E
    R, H, L = 2, 3, 45
    qkv, ref = tc.qkv_case(R, H, L, dtype)
    C = 64 * H
    dense = E.attention(qkv.to(gpu_device), H)
    # a row pitch larger than 3 C: the tensor is the left part of a wider one, whose right part is NaN
    wide = torch.full((R, L, 3 * C + 40), float("nan"), dtype=dtype, device=gpu_device)
    wide[..., :3 * C] = qkv.to(gpu_device)
    view = wide[..., :3 * C]
    assert not view.is_contiguous() and E.attn_takes(view, H)
    assert torch.equal(E.attention(view, H), dense)
    # head 1 of row 0 does not change when every other head's columns, and the other row, are rewritten
    other = (5.0 * torch.randn(R, L, 3 * C, generator=torch.Generator().manual_seed(3))).to(dtype)
    for part in range(3):
        cols = slice(part * C + 64, part * C + 128)
        other[0, :, cols] = qkv[0, :, cols]
    got = E.attention(other.to(gpu_device), H)
    assert torch.equal(got[0, :, 64:128], dense[0, :, 64:128]) and not torch.equal(got[0, :, :64], dense[0, :, :64])
    assert not torch.equal(got[1], dense[1])
    # what the kernel does not take is refused, not computed some other way
    assert not E.attn_takes(qkv.to(gpu_device), 2) and not E.attn_takes(torch.zeros(1, 129, 192, dtype=dtype, device=gpu_device), 1)
    assert not E.attn_takes(qkv.to(gpu_device).float(), H)
    with pytest.raises(E.PwwHipError):
        E.attention(torch.zeros(1, 129, 192, dtype=dtype, device=gpu_device), 1)


# ---- activation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("M,N", [(1, 64), (77, 3072), (154, 4096)])
def test_act(gpu_device, dtype, act, M, N):
    from pww_hip import text_encode as E
    g = torch.Generator().manual_seed(M + N)
    x = (2.0 * torch.randn(M, N, generator=g)).to(dtype)
    big = torch.finfo(dtype).max
    x.view(-1)[:8] = torch.tensor([0.0, -0.0, 60.0, -60.0, big, -big, 1.0, -1.0]).to(dtype)
    pad = 24
    buf = torch.full((M, N + pad), 7.0, dtype=dtype, device=gpu_device)         # a row pitch larger than N
    buf[:, :N] = x.to(gpu_device)
    view = buf[:, :N]
    out = E.act_(view, act)
    assert out.data_ptr() == buf.data_ptr() and (buf[:, N:] == 7.0).all()        # in place, the pad columns untouched
    assert torch.isfinite(out.float()).all()
    stock = E.act_stock(x.to(gpu_device), act)
    ref = tc.act_reference(x, act)
    body = torch.ones(M, N, dtype=torch.bool)
    body.view(-1)[4:6] = False                                                  # the two largest values: compared on their own below
    sel = lambda t: torch.where(body, t.cpu().double(), torch.zeros((), dtype=torch.double))      # noqa: E731
    tc.check(sel(out), sel(stock), sel(ref), "act %s %s M %d N %d" % (act, dtype, M, N))
    flat = out.cpu().reshape(-1)[:8].float()                                    # +-0, +-60, +-max: 0, 0, 60, -0, max, -0
    assert flat[0] == 0 and flat[1] == 0 and flat[2] == 60 and flat[3] == 0 and flat[4] == big and flat[5] == 0
    dense = x.to(gpu_device).clone()
    assert torch.equal(E.act_(dense, act), out)                                 # the pitch changes nothing
