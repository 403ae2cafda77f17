"""Helpers for the GPU parity tests (test infrastructure)."""
import numpy as np
import torch

from oracle import pww_oracle as O

TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}   # per-call bar of BASELINE.md section 4 (x max|O|)


def unfused_inj_forward(module, hidden_states, context=None, mask=None):
    """The reference's op sequence as plain torch ops on the GPU with autocast-like precision
    (half matmuls, fp32 softmax): the 'reference on the same GPU' calibration path."""
    is_dict = isinstance(context, dict)
    ctx = hidden_states if context is None else (context["CONTEXT_TENSOR"] if is_dict else context)
    wdt = module.to_q.weight.dtype
    q = O.split_heads(module.to_q(hidden_states.to(wdt)), module.heads)
    k = O.split_heads(module.to_k(ctx.to(wdt)), module.heads)
    v = O.split_heads(module.to_v(ctx.to(wdt)), module.heads)
    scores = torch.matmul(q, k.transpose(-1, -2))
    bias = 0.0
    if is_dict:
        n = scores.shape[-2]
        try:
            w = context[f"CROSS_ATTENTION_WEIGHT_{n}"]
        except KeyError:        # the reference's fallback (:95-101): resize CROSS_ATTENTION_WEIGHT_ORIG to n tokens, plain torch ops
            w = context["CROSS_ATTENTION_WEIGHT_ORIG"]
            if torch.is_tensor(w):
                ratio = (w.shape[0] * w.shape[1] / n) ** 0.5
                nc = w.shape[2]
                small = torch.nn.functional.interpolate(w.permute(2, 0, 1)[None].float(), scale_factor=1 / ratio, mode="bilinear", align_corners=True)
                w = torch.nn.functional.interpolate(small.reshape(1, nc, -1), size=n, mode="nearest")[0].t()       # [n, nc]
            else:
                w = 0
        bias = context["WEIGHT_FUNCTION"](w, context["SIGMA"], scores)
    probs = ((scores.float() + bias) * module.scale).softmax(dim=-1)
    out = O.merge_heads(torch.matmul(probs.to(v.dtype), v), module.heads)
    return module.to_out[0](out)


def install_unfused(unet):
    for m in unet.modules():
        if m.__class__.__name__ == "CrossAttention":
            m.__class__.__call__ = unfused_inj_forward


def uninstall_all():
    from sd_standin import CrossAttention
    if "__call__" in CrossAttention.__dict__:
        del CrossAttention.__call__


def path_counts(fn, device):
    """fn() under pww_debug_path_counts: its result, and the workgroups of the folded-reference self-attention kernel per path."""
    import ctypes
    from pww_hip import _lib
    lib = _lib.load()
    counts = torch.zeros(4, dtype=torch.int32, device=device)
    lib.pww_debug_path_counts(ctypes.c_void_p(counts.data_ptr()))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.pww_debug_path_counts(None)
    c = counts.tolist()
    return out, {"fast": c[0], "lazy": c[1], "raw": c[3], "exact": c[2]}


def last_attn_route():
    """pww_debug_last_attn_route: the (kind, KS, DT, NW, KG, NSUB, HAS_BIAS, ROWSUM_MFMA, RF) record of this thread's last general attention launch."""
    import ctypes
    from pww_hip import _lib
    rec = (ctypes.c_int32 * 9)()
    assert _lib.load().pww_debug_last_attn_route(rec, 9) == 9
    return tuple(rec)


def rel_l2(a, b):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _blur_exact(mask, sigma, ksize=39):
    """The same Gaussian blur in float64 (fp32 kernel weights as torchvision builds them, reflect padding): what an
    infinitely precise conv2d would return."""
    from pww_hip.ops import gaussian_kernel1d
    k = gaussian_kernel1d(float(sigma), ksize).double().numpy()
    p = ksize // 2
    padded = np.pad(np.asarray(mask, np.float64), p, mode="reflect")
    rows = sum(k[j] * padded[:, j:j + mask.shape[1]] for j in range(ksize))
    return sum(k[j] * rows[j:j + mask.shape[0]] for j in range(ksize))
