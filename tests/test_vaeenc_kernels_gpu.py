"""The three kernels of libpww_hip_vaeenc.so against fp64 on the CPU (vaeenc_cases.py: inputs, references, bars)."""
import pytest
import torch
import torch.nn.functional as F

import vaeenc_cases as C

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


def _name(dtype):
    return str(dtype).split(".")[-1]


# ---- head ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", C.HEAD_VARIANTS)
@pytest.mark.parametrize("shape", C.HEAD_SHAPES)
def test_head_against_fp64(gpu_device, shape, variant, dtype):
    from pww_hip import vae_encode as E
    B, H, W = shape
    u8, image, w, bias = (t.to(gpu_device) for t in C.head_inputs(B, H, W, variant, dtype))
    ref = C.head_reference(B, H, W, variant, dtype)
    stock = F.conv2d(image, w, bias, padding=1)
    assert E.head_takes(image, w, bias) and E.head_takes(u8, w, bias)
    y = E.head(image, w, bias)
    assert tuple(y.shape) == (B, 128, H, W) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    eps = C.check(y, stock, ref, "vaeenc head %s %s %s" % (shape, variant, _name(dtype)))
    # the uint8 form sees the same bits from the table on: the same bytes out; and a second call gives them again
    y8 = E.head(u8, w, bias)
    assert torch.equal(y8, y) and torch.equal(E.head(u8, w, bias), y8) and torch.equal(E.head(image, w, bias), y)
    if variant == "plain" and B * H * W >= 86:
        assert len(torch.unique(u8)) == 256
    if variant == "border":
        # the trap the image is built for: padding with PIXEL 0 (which normalises to -1) lands many bars away on every border pixel
        trap = (C.head_trap(B, H, W, variant, dtype) - ref).abs().amax(1)
        ring = torch.ones(H, W, dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        assert (trap[:, ring] > 10 * eps).all() and (y.double().cpu() - ref).abs().amax(1)[:, ring].max() <= eps


def test_head_declines_what_the_kernel_does_not_take(gpu_device):
    from pww_hip import vae_encode as E
    from pww_hip._lib import PwwHipError
    u8, image, w, bias = (t.to(gpu_device) for t in C.head_inputs(1, 8, 8, "plain", torch.bfloat16))
    assert E.head_takes(image, w, bias)
    assert not E.head_takes(image.float(), w, bias) and not E.head_takes(image.half(), w, bias) and not E.head_takes(image.cpu(), w, bias)
    assert not E.head_takes(image, w[:64], bias[:64]) and not E.head_takes(u8.permute(0, 3, 1, 2), w, bias) and not E.head_takes(image[:, :2], w, bias)
    with pytest.raises(PwwHipError):
        E.head(image.float(), w, bias)
    # the stock restatement takes both forms too (two stock convolutions over differently strided inputs need not agree bit for bit)
    conv = torch.nn.Conv2d(3, 128, 3, padding=1).to(gpu_device, torch.bfloat16)
    with torch.no_grad():
        a, b = E.head_stock(u8, conv), E.head_stock(image, conv)
    assert a.shape == b.shape == (1, 128, 8, 8) and a.is_contiguous(memory_format=torch.channels_last) and b.is_contiguous(memory_format=torch.channels_last)
    assert torch.allclose(a.float(), b.float(), atol=0.05, rtol=0.05)


# ---- down ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plan", [(0, 0), (64, 0), (128, 0), (0, 2)], ids=["auto", "tile64", "tile128", "splitk2"])
@pytest.mark.parametrize("variant", C.DOWN_VARIANTS)
@pytest.mark.parametrize("shape", C.DOWN_SHAPES)
def test_down_against_fp64(gpu_device, shape, variant, plan, dtype):
    from pww_hip import vae_encode as E
    B, H, W, Ch = shape
    x, w, bias = (t.to(gpu_device) for t in C.down_inputs(B, H, W, Ch, variant, dtype))
    x = x.contiguous(memory_format=torch.channels_last)
    ref = C.down_reference(B, H, W, Ch, variant, dtype)
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    assert tuple(ref.shape) == (B, Ch, Ho, Wo)
    stock = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)
    assert E.down_takes(x, w, bias)
    y = E.down(x, w, bias, tile_n=plan[0], splitk=plan[1])
    assert tuple(y.shape) == (B, Ch, Ho, Wo) and y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
    eps = C.check(y, stock, ref, "vaeenc down %s %s tile_n %d splitk %d %s" % (shape, variant, plan[0], plan[1], _name(dtype)))
    assert torch.equal(E.down(x, w, bias, tile_n=plan[0], splitk=plan[1]), y)
    err = (y.double().cpu() - ref).abs().amax(1)
    # the first output row and column read no padding, the last ones (even sizes) read the zero padding: each within the bar on its own
    assert err[:, 0].max() <= eps and err[:, :, 0].max() <= eps and err[:, -1].max() <= eps and err[:, :, -1].max() <= eps
    if variant == "ring":
        # the trap: the symmetric padding of the UNet's downsampler reads a zero where the bright ring is -- many bars away in row 0 and column 0
        trap = (C.down_trap(B, H, W, Ch, variant, dtype) - ref).abs().amax(1)
        assert trap[:, 0].min() > 10 * eps and trap[:, :, 0].min() > 10 * eps


def test_down_declines_what_the_kernel_does_not_take(gpu_device):
    from pww_hip import vae_encode as E
    from pww_hip._lib import PwwHipError
    x, w, bias = (t.to(gpu_device) for t in C.down_inputs(1, 8, 8, 512, "plain", torch.float16))
    cl = x.contiguous(memory_format=torch.channels_last)
    assert E.down_takes(cl, w, bias) and E.down_takes(cl, w)
    assert not E.down_takes(x, w, bias)                                         # NCHW
    assert not E.down_takes(cl[:, :96].contiguous(memory_format=torch.channels_last), w[:, :96], bias)
    assert not E.down_takes(cl[:, :, :1].contiguous(memory_format=torch.channels_last), w, bias) and not E.down_takes(cl, w.float(), bias)
    with pytest.raises(PwwHipError):
        E.down(x, w, bias)
    with pytest.raises(PwwHipError, match="tile_n"):
        E.down(cl, w, bias, tile_n=160)
    y = E.down(cl, w, None)                                                     # no bias: the convolution alone
    assert torch.allclose(y.float(), F.conv2d(F.pad(cl, (0, 1, 0, 1)), w, None, stride=2).float(), atol=0.05, rtol=0.05)


# ---- tail ----------------------------------------------------------------------------------------------------------------------------------
def _tail_on(dev, B, H, W, variant, dtype):
    x, *rest = (t.to(dev) for t in C.tail_inputs(B, H, W, variant, dtype))
    return (x.contiguous(memory_format=torch.channels_last),) + tuple(rest)


def _tail_stock(x, gamma, beta, w, bias, qw, qb, noise):
    """The stock sequence in the storage type: (mean, logvar, z of the mode form, z of the sample form)."""
    m = F.conv2d(F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, 1e-6)), w, bias, padding=1), qw, qb)
    mean, logvar = torch.chunk(m, 2, dim=1)
    logvar = logvar.clamp(-30.0, 20.0)
    return mean, logvar, C.SCALE * mean, C.SCALE * (mean + torch.exp(0.5 * logvar) * noise)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", C.TAIL_VARIANTS)
@pytest.mark.parametrize("shape", C.TAIL_SHAPES)
def test_tail_against_fp64(gpu_device, shape, variant, dtype):
    from pww_hip import vae_encode as E
    B, H, W = shape
    x, gamma, beta, w, bias, qw, qb, noise = _tail_on(gpu_device, B, H, W, variant, dtype)
    ref_mean, ref_logvar, ref_mode, ref_sample = C.tail_reference(B, H, W, variant, dtype)
    s_mean, s_logvar, s_mode, s_sample = _tail_stock(x, gamma, beta, w, bias, qw, qb, noise)
    what = "vaeenc tail %s %s %s" % (shape, variant, _name(dtype))
    sampled = variant == "sample"
    args = (x, gamma, beta, w, bias, qw, qb, noise if sampled else None)
    assert E.tail_takes(*args)
    moments, z = E.tail(*args, eps=1e-6, scale=C.SCALE)
    assert tuple(moments.shape) == (B, 8, H, W) and tuple(z.shape) == (B, 4, H, W) and moments.dtype == z.dtype == torch.float32
    eps = C.check(moments[:, :4], s_mean, ref_mean, what + " mean")
    C.check(moments[:, 4:], s_logvar, ref_logvar, what + " logvar")
    if sampled:
        C.check(z, s_sample, ref_sample, what + " z (sample)")
    else:
        C.check(z, s_mode, ref_mode, what + " z (mode)")
        assert torch.equal(z, C.SCALE * moments[:, :4])                         # the mode form IS scale * mean
    # bitwise repeatable, and the moments are optional
    again, z2 = E.tail(*args, eps=1e-6, scale=C.SCALE)
    none, z3 = E.tail(*args, eps=1e-6, scale=C.SCALE, moments=False)
    assert torch.equal(again, moments) and torch.equal(z2, z) and none is None and torch.equal(z3, z)
    assert moments[:, 4:].min() >= -30 and moments[:, 4:].max() <= 20
    if variant == "clamp" and H * W >= 64:
        assert (ref_logvar == -30).any() and (ref_logvar == 20).any() and (moments[:, 4:] == -30).any() and (moments[:, 4:] == 20).any()
    if variant == "border" and H * W >= 64:
        # the trap the input is built for: padding the INPUT with zeros (which the norm turns into about +8) lands many bars away
        assert (C.tail_trap(B, H, W, variant, dtype) - ref_mean).abs().max().item() > 10 * eps


@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_statistics_are_bitwise_repeatable(gpu_device, dtype):
    from pww_hip import vae_encode as E
    for B, H, W in C.TAIL_SHAPES:
        x = _tail_on(gpu_device, B, H, W, "border", dtype)[0]
        first = E.tail_statistics(x).clone()
        second = E.tail_statistics(x)
        assert torch.equal(first, second) and first.dtype == torch.float32 and first.shape[0] == B and tuple(first.shape[2:]) == (32, 2)
        # ... and they are the moments: chunks added up, against fp64
        xd = C.tail_inputs(B, H, W, "border", dtype)[0].double().reshape(B, 32, -1)
        tot = first.double().sum(1).cpu()
        assert torch.allclose(tot[..., 0], xd.sum(-1), rtol=1e-5, atol=1e-3) and torch.allclose(tot[..., 1], (xd * xd).sum(-1), rtol=1e-5, atol=1e-3)


def test_tail_declines_what_the_kernel_does_not_take(gpu_device):
    from pww_hip import vae_encode as E
    from pww_hip._lib import PwwHipError
    x, gamma, beta, w, bias, qw, qb, noise = _tail_on(gpu_device, 1, 8, 8, "sample", torch.bfloat16)
    assert E.tail_takes(x, gamma, beta, w, bias, qw, qb, noise) and E.tail_takes(x, gamma, beta, w, bias, qw.reshape(8, 8), qb)
    assert not E.tail_takes(x.contiguous(), gamma, beta, w, bias, qw, qb)       # NCHW
    assert not E.tail_takes(x[:, :128].contiguous(memory_format=torch.channels_last), gamma[:128], beta[:128], w[:, :128], bias, qw, qb)
    assert not E.tail_takes(x, gamma, beta, w.float(), bias, qw, qb) and not E.tail_takes(x, gamma, beta, w, bias, qw, qb, groups=16)
    assert not E.tail_takes(x, gamma, beta, w, bias, qw, qb, noise[:, :2]) and not E.tail_takes(x, gamma, beta, w, bias, qw, qb, noise.float())
    with pytest.raises(PwwHipError):
        E.tail(x.contiguous(), gamma, beta, w, bias, qw, qb)
