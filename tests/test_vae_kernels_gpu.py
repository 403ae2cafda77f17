"""The two kernels of libpww_hip_vae.so against fp64 on the CPU (vae_cases.py: inputs, references, bars)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import vae_cases as C

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


def _run_attention(q, k, v, variant, dev):
    from pww_hip import vae as V
    q, k, v = (t.to(dev) for t in (q, k, v))
    if variant == "separate":
        return V.attention(q, k, v), V.attention_stock(q, k, v)
    # the three slices of one [B, N, 1536] tensor, read where they lie; the rows behind the last token hold NaN
    B, N, D = q.shape
    buf = torch.full((B, N + 3, 3 * D), float("nan"), dtype=q.dtype, device=dev)
    buf[:, :N, :D], buf[:, :N, D:2 * D], buf[:, :N, 2 * D:] = q, k, v
    qs, ks, vs = buf[:, :N, :D], buf[:, :N, D:2 * D], buf[:, :N, 2 * D:]
    assert qs.stride(1) == 3 * D and ks.data_ptr() == buf.data_ptr() + 2 * D and V.attention_takes(qs, ks, vs)
    return V.attention(qs, ks, vs), V.attention_stock(q, k, v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", C.ATTN_VARIANTS)
@pytest.mark.parametrize("shape", C.ATTN_SHAPES)
def test_attention_against_fp64(gpu_device, shape, variant, dtype):
    B, N = shape
    q, k, v = C.attn_inputs(B, N, variant, dtype)
    ref = C.attn_reference(B, N, variant, dtype)
    native, stock = _run_attention(q, k, v, variant, gpu_device)
    assert tuple(native.shape) == (B, N, 512) and native.dtype == dtype and torch.isfinite(native).all()
    ratio, over = C.attn_row_check(native, stock, ref)
    print("vae attention B %d N %d %s %s: worst row at %.3f of its bar" % (B, N, variant, dtype, ratio))
    assert not over, over[:8]
    if variant == "spike" and N > 1:
        # the probes do what they are for: without its probe key a probe row would sit many bars away
        rows = C.probe_rows(N)
        err_stock = (stock.double().cpu() - ref).abs().amax(-1)[0, rows]
        bar = 1.5 * err_stock + 2e-3 * ref.abs().amax(-1)[0, rows]
        qd, kd, vd = (t[0].double() for t in (q, k, v))
        logits = qd[rows] @ kd.T * 512 ** -0.5
        top = logits.argmax(-1)
        logits[torch.arange(len(rows)), top] = -float("inf")
        dropped = torch.softmax(logits, -1) @ vd if N > 1 else None
        moved = (dropped - ref[0, rows]).abs().amax(-1)
        assert (moved > 10 * bar).all(), (moved / bar).tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_hot_logits(gpu_device, dtype):
    B, N = 1, 100
    q, k, v = C.attn_inputs(B, N, "hot", dtype)
    logits = torch.bmm(q.double(), k.double().transpose(1, 2)) * 512 ** -0.5
    assert 6.0 < logits.std().item() < 10.0
    native, stock = _run_attention(q, k, v, "sliced", gpu_device)
    ratio, over = C.attn_row_check(native, stock, C.attn_reference(B, N, "hot", dtype))
    print("vae attention hot logits %s: worst row at %.3f of its bar" % (dtype, ratio))
    assert not over, over[:8]


def test_attention_writes_the_channels_last_tensor_in_place(gpu_device):
    """`out` may be the [B, H W, 512] view of a channels_last [B, 512, H, W] tensor."""
    from pww_hip import vae as V
    q, k, v = (t.to(gpu_device) for t in C.attn_inputs(1, 100, "separate", torch.bfloat16))
    y = torch.zeros(1, 512, 10, 10, dtype=torch.bfloat16, device=gpu_device).contiguous(memory_format=torch.channels_last)
    V.attention(q, k, v, out=y.permute(0, 2, 3, 1).reshape(1, 100, 512))
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(1, 100, 512), V.attention(q, k, v))


def test_attention_error_paths_make_no_launch(gpu_device):
    from pww_hip import _lib
    lib = _lib.load_vae()
    dev = gpu_device
    q, k, v = (torch.randn(1, 40, 520, device=dev).to(torch.float16) for _ in range(3))
    o = torch.full((1, 40, 520), 7.0, dtype=torch.float16, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def desc(D=512, rs=520):
        return _lib.VaeAttnDesc(ctypes.sizeof(_lib.VaeAttnDesc), _lib.DTYPE_F16, 1, 40, D, 0.0, 40 * 520, rs, 40 * 520, rs, 40 * 520, rs, 40 * 520, rs)

    cases = (("null pointer", lambda: lib.pww_vae_attn_fwd(p(q), None, p(v), p(o), ctypes.byref(desc()), stream), _lib.PWW_EINVAL),
             ("head dim", lambda: lib.pww_vae_attn_fwd(p(q), p(k), p(v), p(o), ctypes.byref(desc(D=256)), stream), _lib.PWW_ENOTSUP),
             ("row stride", lambda: lib.pww_vae_attn_fwd(p(q), p(k), p(v), p(o), ctypes.byref(desc(rs=516)), stream), _lib.PWW_ENOTSUP))
    for what, call, code in cases:
        rc = call()
        assert rc == code, (what, rc)
        assert lib.pww_last_error(), what
        torch.cuda.synchronize()
        assert (o == 7.0).all(), what
    # ... and the same descriptor with good arguments runs
    assert lib.pww_vae_attn_fwd(p(q), p(k), p(v), p(o), ctypes.byref(desc()), stream) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o[:, :, :512]).all() and (o[:, :, 512:] == 7.0).all() and not (o[:, :, :512] == 7.0).all()
    # the wrapper declines what the library would
    from pww_hip import vae as V
    assert not V.attention_takes(q[:, :, :256], k[:, :, :256], v[:, :, :256]) and not V.attention_takes(q[:, :, 4:516], k[:, :, 4:516], v[:, :, 4:516])
    with pytest.raises(_lib.PwwHipError):
        V.attention(q[:, :, :256], k[:, :, :256], v[:, :, :256])


def _tail_on(dev, B, H, W, variant, dtype):
    x, gamma, beta, w, bias = (t.to(dev) for t in C.tail_inputs(B, H, W, variant, dtype))
    return x.contiguous(memory_format=torch.channels_last), gamma, beta, w, bias


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", C.TAIL_VARIANTS)
@pytest.mark.parametrize("shape", C.TAIL_SHAPES)
def test_tail_against_fp64(gpu_device, shape, variant, dtype):
    from pww_hip import vae as V
    B, H, W = shape
    x, gamma, beta, w, bias = _tail_on(gpu_device, B, H, W, variant, dtype)
    ref = C.tail_reference(B, H, W, variant, dtype)
    stock = F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, 1e-6)), w, bias, padding=1)
    what = "vae tail %s %s %s" % (shape, variant, str(dtype).split(".")[-1])
    sample = V.tail(x, gamma, beta, w, bias, 1e-6, "sample")
    assert tuple(sample.shape) == (B, 3, H, W) and sample.dtype == dtype and sample.is_contiguous()
    eps = C.check_sample(sample, stock, ref, what)
    u8 = V.tail(x, gamma, beta, w, bias, 1e-6, "uint8")
    C.check_uint8(u8, ref, eps, what)
    if variant == "saturate" and H * W >= 64:
        want = 255.0 * (ref / 2 + 0.5).clamp(0, 1)
        assert (want == 0).any() and (want == 255).any() and (u8 == 0).any() and (u8 == 255).any()
    if variant == "border" and H * W >= 64:
        # the trap the input is built for: padding the INPUT with zeros (which the norm turns into +8) lands many bars away
        xd, g, b_, wd, bd = (t.double() for t in C.tail_inputs(B, H, W, variant, dtype))
        mean = xd.reshape(B, 32, -1).mean(-1)
        var = xd.reshape(B, 32, -1).var(-1, unbiased=False)
        xp = F.pad(xd, (1, 1, 1, 1))
        a = (xp.reshape(B, 32, 4, H + 2, W + 2) - mean[:, :, None, None, None]) / (var[:, :, None, None, None] + 1e-6).sqrt()
        trap = F.conv2d(F.silu(a.reshape(B, 128, H + 2, W + 2) * g[None, :, None, None] + b_[None, :, None, None]), wd, bd)
        assert (trap - ref).abs().max().item() > 10 * eps


@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_statistics_are_bitwise_repeatable(gpu_device, dtype):
    from pww_hip import vae as V
    for B, H, W in C.TAIL_SHAPES:
        x = _tail_on(gpu_device, B, H, W, "border", dtype)[0]
        first = V.tail_moments(x).clone()
        second = V.tail_moments(x)
        assert torch.equal(first, second) and first.dtype == torch.float32 and first.shape[0] == B and tuple(first.shape[2:]) == (32, 2)
        # ... and they are the moments: chunks added up, against fp64
        xd = C.tail_inputs(B, H, W, "border", dtype)[0].double().reshape(B, 32, -1)
        tot = first.double().sum(1).cpu()
        assert torch.allclose(tot[..., 0], xd.sum(-1), rtol=1e-5, atol=1e-4) and torch.allclose(tot[..., 1], (xd * xd).sum(-1), rtol=1e-5, atol=1e-4)
        # two runs of the whole tail agree bit for bit, too
        _, gamma, beta, w, bias = _tail_on(gpu_device, B, H, W, "border", dtype)
        assert torch.equal(V.tail(x, gamma, beta, w, bias, 1e-6, "uint8"), V.tail(x, gamma, beta, w, bias, 1e-6, "uint8"))


def test_tail_declines_what_the_kernel_does_not_take(gpu_device):
    from pww_hip import vae as V
    from pww_hip._lib import PwwHipError
    x, gamma, beta, w, bias = _tail_on(gpu_device, 1, 8, 8, "plain", torch.bfloat16)
    assert V.tail_takes(x, gamma, beta, w, bias)
    assert not V.tail_takes(x.contiguous(), gamma, beta, w, bias)                       # NCHW
    assert not V.tail_takes(x[:, :64].contiguous(memory_format=torch.channels_last), gamma[:64], beta[:64], w[:, :64], bias)
    assert not V.tail_takes(x, gamma, beta, w.float(), bias) and not V.tail_takes(x, gamma, beta, w, bias, groups=16)
    with pytest.raises(PwwHipError):
        V.tail(x.contiguous(), gamma, beta, w, bias)
    with pytest.raises(PwwHipError):
        V.tail(x, gamma, beta, w, bias, output="float")
