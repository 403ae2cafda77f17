"""Inputs, references and bars of the AutoencoderKL decode tests (test_vae_host.py, test_vae_kernels_gpu.py, test_vae_decode_gpu.py and the
child process vae_decode_child.py).

The reference everywhere is stock torch on the same (rounded) weights and inputs, upcast: fp64 on the CPU for the two kernels, fp32 for the
whole decoder. The rule of every comparison is the one of the fused attention (test_attention_gpu.py):

    err(native vs reference) <= 1.5 * err(stock same-dtype op sequence vs reference) + 2e-3 * max|reference|

measured per case against the stock path, never against the code under test. For the attention kernel it is taken per query row. The uint8
form has a derived bar: a correctly rounded quantisation of a value within eps of y_ref lies within 0.5 + 127.5 eps of
255 * clamp(y_ref / 2 + 0.5, 0, 1), at every pixel.
"""
import functools

import torch

D = 512
ATTN_SHAPES = ((1, 1), (1, 16), (1, 100), (2, 1024))        # (B, N): one row; less than a block; ragged on both axes; 32 key blocks, 2 images
ATTN_VARIANTS = ("separate", "sliced", "spike")
PROBE_LOGIT, V_STD, V_PROBE, HOT_STD = 6.0, 0.125, 4.0, 8.0
TAIL_SHAPES = ((1, 1, 1), (1, 8, 8), (1, 24, 40), (2, 64, 64))     # (B, H, W)
TAIL_VARIANTS = ("plain", "border", "saturate")
DECODE_LATENTS = ((1, 4, 8, 8), (2, 4, 8, 12))
ODD_LATENT = (1, 4, 5, 7)


def probe_rows(N):
    return sorted({r for r in (0, 31, 32, N - 2, N - 1) if 0 <= r < N})


def probe_keys(N):
    """N - 1, N - 2, key 0, the first key of the last 32-key block."""
    return [m for m in (N - 1, N - 2, 0, (N - 1) // 32 * 32) if m >= 0]


@functools.lru_cache(maxsize=None)
def attn_inputs(B, N, variant, dtype):
    """q, k, v [B, N, 512] in `dtype` on the CPU. Gaussian q and k (scaled logits of unit spread), v of spread V_STD. `spike`: each probe row
    points at ONE key with a scaled logit of PROBE_LOGIT (the query row parallel to the rounded key), whose v row is V_PROBE -- dropping that
    key, or masking it wrongly, moves the row by about its share times 4. `hot`: the logits have a spread of HOT_STD."""
    g = torch.Generator().manual_seed(4321 + 7 * N + B)
    q, k = torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    v = torch.randn(B, N, D, generator=g) * V_STD
    if variant == "hot":
        q = q * HOT_STD
    kT = k.to(dtype).float()
    if variant == "spike":
        keys = probe_keys(N)
        for b in range(B):
            for i, r in enumerate(probe_rows(N)):
                kp = kT[b, keys[(i + b) % len(keys)]]
                q[b, r] = kp * (PROBE_LOGIT / (D ** -0.5 * (kp * kp).sum()))
            v[b, sorted(set(keys))] = V_PROBE
    return q.to(dtype), kT.to(dtype), v.to(dtype)


@functools.lru_cache(maxsize=None)
def attn_reference(B, N, variant, dtype):
    """fp64 on the CPU: O [B, N, 512]."""
    q, k, v = (t.double() for t in attn_inputs(B, N, variant, dtype))
    return torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * D ** -0.5, dim=-1), v)


def attn_row_check(native, stock, ref):
    """Per-row errors and bars; returns (worst ratio err / bar, rows over the bar)."""
    err = (native.double().cpu() - ref).abs().amax(-1)
    err_stock = (stock.double().cpu() - ref).abs().amax(-1)
    bar = 1.5 * err_stock + 2e-3 * ref.abs().amax(-1)
    over = (err > bar).nonzero().tolist()
    ratio = (err / bar.clamp_min(1e-300)).max().item() if not over else float("inf")
    return ratio, over


@functools.lru_cache(maxsize=None)
def tail_inputs(B, H, W, variant, dtype):
    """x [B, 128, H, W] (NCHW on the CPU), gamma, beta [128], w [3, 128, 3, 3], bias [3] in `dtype`.
    border: the image sits at -2 with a spread of 0.25 and its border ring one higher, so that a zero of the INPUT would be +8 after the norm:
    padding the input instead of the activation moves every border pixel by many bars. saturate: a weight spread that drives y past +-1."""
    g = torch.Generator().manual_seed(977 + 13 * H + W + B)
    x = torch.randn(B, 128, H, W, generator=g)
    if variant == "border":
        x = x * 0.25 - 2.0
        ring = torch.ones(H, W, dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        x[:, :, ring] += 1.0
    x = x + 0.3 * torch.randn(B, 128, 1, 1, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    w = torch.randn(3, 128, 3, 3, generator=g) * (0.1 if variant == "saturate" else 0.03)
    bias = 0.1 * torch.randn(3, generator=g)
    return tuple(t.to(dtype) for t in (x, gamma, beta, w, bias))


@functools.lru_cache(maxsize=None)
def tail_reference(B, H, W, variant, dtype, eps=1e-6):
    """fp64 on the CPU: y [B, 3, H, W]."""
    import torch.nn.functional as F
    x, gamma, beta, w, bias = (t.double() for t in tail_inputs(B, H, W, variant, dtype))
    return F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, eps)), w, bias, padding=1)


def sample_bar(stock, ref):
    """eps of the rule above for one case (global maximum norm)."""
    return 1.5 * (stock.double().cpu() - ref.double().cpu()).abs().max().item() + 2e-3 * ref.abs().max().item()


def check_sample(native, stock, ref, what):
    eps = sample_bar(stock, ref)
    err = (native.double().cpu() - ref.double().cpu()).abs().max().item()
    print("%s: sample err %.3e, bar %.3e (stock err %.3e, max|ref| %.3e)" % (what, err, eps, (eps - 2e-3 * ref.abs().max().item()) / 1.5, ref.abs().max().item()))
    assert err <= eps, (what, err, eps)
    return eps


def check_uint8(u8, ref, eps, what):
    """u8 [B, H, W, 3] against the reference sample [B, 3, H, W]: every pixel within the derived bar."""
    want = 255.0 * (ref.double().cpu() / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == tuple(want.shape), (what, u8.dtype, u8.shape)
    err = (u8.cpu().double() - want).abs().max().item()
    print("%s: uint8 err %.3f, bar %.3f" % (what, err, 0.5 + 127.5 * eps))
    assert err <= 0.5 + 127.5 * eps, (what, err, eps)


def make_vae(dtype, device):
    from sd_standin import AutoencoderKL
    return AutoencoderKL().to(device=device, dtype=dtype).eval()


def latent(shape, dtype, device):
    g = torch.Generator().manual_seed(55 + shape[2] * 31 + shape[3])
    return torch.randn(*shape, generator=g).to(device=device, dtype=dtype)


def decode_reference(vae, z):
    """The fp32 decoder on the same weights, upcast, on z's device: [B, 3, 8 h, 8 w] fp32."""
    import copy
    ref = copy.deepcopy(vae).float()
    with torch.no_grad():
        return ref.decode(z.float()).sample


def decode_checks(vae, shape, dtype, device):
    """One multiple-of-8 case: both forms of pww_hip.vae.decode against the fp32 decoder under the bars above; returns stats() of the two
    native calls."""
    from pww_hip import vae as V
    z = latent(shape, dtype, device)
    with torch.no_grad():
        ref = decode_reference(vae, z)
        stock = vae.decode(z).sample
    V.reset_stats()
    sample = V.decode(vae, z, "sample")
    u8 = V.decode(vae, z, "uint8")
    st = V.stats()
    what = "decode %s %s" % (tuple(shape), str(dtype).split(".")[-1])
    assert tuple(sample.shape) == tuple(ref.shape) and sample.dtype == dtype
    eps = check_sample(sample, stock, ref, what)
    check_uint8(u8, ref, eps, what)
    return st


# 14 resnets (2 in the mid block, 3 in each of the 4 up blocks), 2 of them with a shortcut (512 -> 256, 256 -> 128); 2 norms each + the attention's
SD_COUNTS = {"resnet_plain": 12, "resnet_shortcut": 2, "upsample": 3, "norms": 2 * 14 + 1}


def assert_native(st, calls, attn=True, tail=True):
    """`calls` decodes of the SD configuration with everything on the native path (but what a switch turned off)."""
    assert st["decodes"] == calls
    assert st["conv3x3"] == {"native": calls * (2 * SD_COUNTS["resnet_plain"] + SD_COUNTS["resnet_shortcut"]), "stock": 0}, st
    assert st["conv_shortcut"] == {"native": calls * SD_COUNTS["resnet_shortcut"], "stock": 0}, st
    assert st["upsample"] == {"native": calls * SD_COUNTS["upsample"], "stock": 0}, st
    assert st["group_norm"] == {"native": calls * SD_COUNTS["norms"], "stock": 0}, st
    assert st["attention"] == ({"native": calls, "stock": 0} if attn else {"native": 0, "stock": calls}), st
    assert st["tail"] == ({"native": calls, "stock": 0} if tail else {"native": 0, "stock": calls}), st
