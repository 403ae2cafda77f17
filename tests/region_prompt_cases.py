"""The region-prompts fixture shared by tests/test_region_prompts_host.py and tests/test_region_prompts_gpu.py (test infrastructure): its
constants, the numpy restatements of the two launches of libpww_hip_regions.so (include/pww_hip_regions.h) and the fp32 CPU loop built from
the oracle's pieces that both files compare against. Nothing in here calls the code under test."""
import math
import os

import numpy as np
import torch

import pww_cases as cases
from gpu_util import uninstall_all
from negative_cases import CAP  # noqa: F401  (the loop caps: tests/test_loop_gpu.py::test_tiny_loop_vs_reference)
from oracle import pww_oracle as O

# ---- the fixture: the runner example, a full prompt for each of its five colours
REGIONS = {(13, 255, 0): "an old oak tree with autumn leaves", (255, 255, 255): "a white fluffy dog, studio photo",
           (90, 206, 255): "stormy sky with dark clouds", (0, 0, 0): "a black cat sleeping", (74, 18, 1): "wet cobblestone street at night"}
QK_GAIN = 4.0
STEPS = 10
GUIDANCE = 7.5
ALT_SCALES = (15.0, 2.0, 15.0, 2.0, 15.0)
ORACLE_VISIBLE = 0.379         # CPU-measured rel-L2(with, without) of the oracle loop (profiles/region_prompts.md; the host test re-measures it)


def rotated(regions=REGIONS):
    """The same colours, every prompt moved on by one colour."""
    colors, prompts = list(regions), list(regions.values())
    return dict(zip(colors, prompts[1:] + prompts[:1]))


def with_scales(scales, regions=REGIONS, weight=1.0):
    return {c: (p, weight, s) for (c, p), s in zip(regions.items(), scales)}


# ---- numpy restatements (fp32, one operation at a time, in the header's order)

def box_masks(rgb, colors):
    """[K, H // 8, W // 8] fp32: the share of each 8 x 8 pixel block that has the colour exactly (a multiple of 1 / 64)."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[0] // 8, rgb.shape[1] // 8
    out = []
    for c in colors:
        eq = (rgb[:8 * h, :8 * w] == np.array(c, dtype=rgb.dtype)).all(-1)
        out.append(eq.reshape(h, 8, w, 8).sum(axis=(1, 3)).astype(np.float32) * np.float32(1.0 / 64.0))
    return np.stack(out)


def _feather_axis(plane, taps, axis):
    """One pass along `axis`: taps in ascending x, the sum divided by the sum of the taps that fall inside the plane."""
    plane = np.moveaxis(plane, axis, -1)
    n, radius = plane.shape[-1], len(taps) - 1
    acc, norm = np.zeros_like(plane), np.zeros_like(plane)
    for x in range(-radius, radius + 1):
        lo, hi = max(0, -x), min(n, n - x)             # positions p with 0 <= p + x < n
        if lo >= hi:
            continue
        t = taps[abs(x)]
        acc[..., lo:hi] = acc[..., lo:hi] + t * plane[..., lo + x:hi + x]
        norm[..., lo:hi] = norm[..., lo:hi] + t
    return np.moveaxis(acc / norm, -1, axis)


def feather(planes, sigma):
    """The separable Gaussian of pww_regions_masks over [K, h, w] fp32 planes: along the rows, then along the columns."""
    if not sigma > 0:
        return planes
    radius = int(math.ceil(3.0 * sigma))
    taps = np.exp(-0.5 * (np.arange(radius + 1, dtype=np.float64) / sigma) ** 2).astype(np.float32)
    return _feather_axis(_feather_axis(planes.astype(np.float32), taps, 2), taps, 1)


def region_masks(rgb, colors, sigma=0.0):
    return feather(box_masks(rgb, colors), sigma)


def region_weights(weights, beta):
    """a_k = weight_k (1 - beta), formed in fp32."""
    return (np.float32(1.0) - np.float32(beta)) * np.asarray(weights, dtype=np.float32)


def blend(eps, masks, weights, scales, g):
    """pww_regions_combine: eps [(K + 2) n, C, h, w] (any float dtype; read as fp32), masks [n, K, h, w], weights / scales [n, K] -> fp32
    [n, C, h, w]; rows [base x n, region 1 x n, ..., region K x n, unconditional x n]."""
    masks, weights, scales = (np.asarray(a, dtype=np.float32) for a in (masks, weights, scales))
    n, K = masks.shape[:2]
    e = np.asarray(eps, dtype=np.float32).reshape((K + 2, n) + tuple(eps.shape[1:]))
    g = np.float32(g)
    out = np.empty(e.shape[1:], dtype=np.float32)
    for i in range(n):
        u = e[K + 1, i]
        wk = [weights[i, k] * masks[i, k] for k in range(K)]
        total = wk[0]
        for k in range(1, K):
            total = total + wk[k]
        acc = u + ((np.float32(1.0) - total) * g)[None] * (e[0, i] - u)
        for k in range(K):
            acc = acc + (wk[k] * scales[i, k])[None] * (e[k + 1, i] - u)
        out[i] = acc
    return out


def entries(regions, guidance=GUIDANCE):
    """{colour: prompt | (prompt, weight, scale)} -> colours, prompts, weights, scales (None resolved to the call's)."""
    colors, prompts, weights, scales = [], [], [], []
    for c, v in regions.items():
        v = (v,) if isinstance(v, str) else tuple(v)
        colors.append(c), prompts.append(v[0]), weights.append(v[1] if len(v) > 1 else 1.0)
        scales.append(guidance if len(v) < 3 or v[2] is None else v[2])
    return colors, prompts, weights, scales


# ---- the oracle loop

def region_dict(text, tok, rgb, prompt):
    """The dict of a region prompt: the UNCONDITIONAL dict the oracle's builder returns when the region's prompt is passed as its
    unconditional prompt (the integer 0 in every weight slot: plain cross-attention)."""
    return O.encode_text_color_inputs(text, tok, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, prompt)[3]


def oracle_loop(regions, beta=0.0, sigma=0.0, steps=STEPS, seed=0, guidance=GUIDANCE, wf=cases.weight_fn_runner, config="tiny", qk_gain=QK_GAIN):
    """fp32 CPU: the reference's loop with K more batch-1 evaluations per step -- the region dicts, evaluated with the zero lambda like the
    unconditional pass -- and `blend` where the reference combines guidance. regions None / {}: the reference's loop."""
    vae, unet, text, tok, sch = cases.build_tools(config, qk_gain=qk_gain)
    rgb = cases.load_example_rgb()
    O.install_oracle_attention(unet)
    try:
        extra_seeds, table, cond, uncond = O.encode_text_color_inputs(text, tok, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "")
        zero = lambda w, sigma, qk: 0.0      # noqa: E731
        rdicts = []
        if regions:
            colors, prompts, weights, scales = entries(regions, guidance)
            rdicts = [region_dict(text, tok, rgb, p) for p in prompts]
            masks = region_masks(rgb, colors, sigma)[None]
            a, s = region_weights(weights, beta)[None], np.asarray(scales, dtype=np.float32)[None]
        latents = O.initial_latents(seed, 4, rgb.shape[0], rgb.shape[1], table, extra_seeds)
        sch.set_timesteps(steps)
        latents = latents * sch.init_noise_sigma
        with torch.no_grad():
            for i, t in enumerate(sch.timesteps):
                sigma_t = sch.sigmas[i]
                x = sch.scale_model_input(latents, t)
                cond.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": wf})
                rows = [unet(x, t, encoder_hidden_states=cond).sample]
                for d in rdicts + [uncond]:
                    d.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": zero})
                    rows.append(unet(x, t, encoder_hidden_states=d).sample)
                if rdicts:
                    noise = torch.from_numpy(blend(torch.cat(rows).numpy(), masks, a, s, guidance))
                else:
                    noise = O.cfg_combine(rows[0], rows[1], guidance)
                latents = sch.step(noise, t, latents).prev_sample
        return latents
    finally:
        uninstall_all()


# ---- the oracle loop's recorded latents
# An oracle loop is 10 steps x 7 fp32 UNet evaluations on the CPU, most of a minute; the GPU tests compare against five of them. They are
# recorded once (`python tests/region_prompt_cases.py`) in tests/golden/region_prompts_oracle.npz; tests/test_region_prompts_host.py runs the
# loops again and holds the record to them ("with" / "without" in every run, the others under PWW_SLOW=1).
GOLDEN = os.path.join(cases.GOLDEN, "region_prompts_oracle.npz")
RECORDED = {"with": dict(regions=REGIONS), "without": dict(regions=None), "rotated": dict(regions=rotated()),
            "scales": dict(regions=with_scales(ALT_SCALES)), "beta": dict(regions=REGIONS, beta=0.5)}
GOLDEN_TOL = 1e-4         # rel-L2 between two fp32 CPU runs of one loop (thread count and BLAS blocking change the summation order)


def recorded():
    """name -> final latent [1, 4, 64, 64] of oracle_loop(**RECORDED[name])."""
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in RECORDED}


# ---- CPU stand-ins for the host tests

def cpu_region_masks(rgb, colors, feather=0.0):
    """ops.region_masks for tensors on the CPU: the numpy restatement."""
    return torch.from_numpy(np.ascontiguousarray(region_masks(rgb.numpy(), colors, feather)))


def folded_forward(module, hidden_states, context=None, mask=None):
    """fp32 torch restatement of what the cross-attention launches compute for a (folded) dict context: per image b,
    bias_b = gate[b] * weight_function(w_b, sigma, scores_b) with the image's own scores, added before the scale."""
    from pww_hip.attention import ROW_GATE
    if not isinstance(context, dict):
        return O.inj_forward(module, hidden_states, context)
    h, ctx, gate = module.heads, context["CONTEXT_TENSOR"], context.get(ROW_GATE)
    outs = []
    for b in range(hidden_states.shape[0]):
        q, k, v = (O.split_heads(torch.nn.functional.linear(x[b:b + 1], m.weight), h)
                   for x, m in ((hidden_states, module.to_q), (ctx, module.to_k), (ctx, module.to_v)))
        scores = torch.matmul(q, k.transpose(-1, -2))
        w = context["CROSS_ATTENTION_WEIGHT_%d" % scores.shape[-2]]
        if torch.is_tensor(w) and w.dim() == 4:
            w = w[b, 0]
        bias = context["WEIGHT_FUNCTION"](w, context["SIGMA"], scores)
        if gate is not None:
            bias = bias * gate[b]
        outs.append(O.merge_heads(torch.matmul(((scores + bias) * module.scale).softmax(dim=-1), v), h))
    return torch.nn.functional.linear(torch.cat(outs), module.to_out[0].weight, module.to_out[0].bias)


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **{name: oracle_loop(**kw).numpy() for name, kw in RECORDED.items()})
    print("wrote", GOLDEN)
