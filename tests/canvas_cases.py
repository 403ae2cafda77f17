"""The canvas fixture shared by tests/test_canvas_host.py and tests/test_canvas_gpu.py (test infrastructure): the window grids of the cases,
numpy fp32 restatements of the two launches of libpww_hip_canvas.so (include/pww_hip_canvas.h) with the same operation order, and the fp32
CPU canvas loop built from the oracle's pieces that both files compare against. Nothing in here calls the code under test."""
import math
import os

import numpy as np
import torch

import pww_cases as cases
import region_prompt_cases as R
from gpu_util import uninstall_all
from oracle import pww_oracle as O

# the project's loop bars for this feature: rel-L2 of the final latent against the fp32 oracle loop
CAP = {torch.float16: 1e-2, torch.bfloat16: 5e-2}
UNFUSED_SLACK = (1.5, 2e-3)        # ... and at most 1.5 x the drift of the unfused torch path on the same GPU + 2e-3


# ---- the window grid

def windows(L, win, stride):
    """The origins along an axis of latent length L: 0, s, 2 s, ... below L - win, followed by L - win."""
    out, o = [], 0
    while o < L - win:
        out.append(o)
        o += stride
    return out + [L - win]


def grid(Hc, Wc, win, stride):
    return windows(Hc, win, stride), windows(Wc, win, stride)


# the kernel cases: (canvas latent, window, stride)
KERNEL_CASES = {"a": ((8, 20), 8, 4),          # one axis, aligned origins
                "b": ((12, 11), 8, 4),         # two axes, an odd clamped origin, an odd pitch
                "c": ((64, 256), 64, 32),      # the product shape: seven windows, the 16-byte path
                "d": ((16, 16), 16, 8),        # window = canvas: ny = nx = 1
                # two more where the combine changes its path: a row pitch and a window that allow 16-byte accesses ...
                "f": ((8, 24), 8, 4),          # ... but origins that are no multiples of 8: one pixel per lane
                "g": ((24, 32), 16, 8)}        # ... and origins that are: the 16-byte path on two axes, more than one covering window per axis


# ---- numpy / torch-CPU restatements (fp32, one operation at a time, in the header's order)

def gather(canvas, ys, xs, h, w, denom, copies, dtype):
    """pww_canvas_gather: canvas fp32 [C, Hc, Wc] (torch, CPU) -> `dtype` [copies * n_w, C, h, w]: indexing, one fp32 division (by an fp32
    tensor: IEEE division, no reciprocal), one rounding."""
    d = torch.tensor(float(np.float32(denom)), dtype=torch.float32)
    rows = [(canvas[:, y0:y0 + h, x0:x0 + w] / d).to(dtype) for y0 in ys for x0 in xs]
    return torch.stack(rows * copies)


def ramp_weights(L, ramp):
    """r_L(l), l = 0 .. L - 1, as integers."""
    l = np.arange(L)
    return np.ones(L, dtype=np.int64) if ramp == 0 else np.minimum(np.minimum(l, L - 1 - l) + 1, ramp)


def combine(eps, ys, xs, canvas_hw, g, ramp=0, masks=None, weights=None, scales=None):
    """pww_canvas_combine: eps [(K + 2) n_w, C, h, w] (any float dtype; read as fp32) -> fp32 [C, Hc, Wc]. Windows are accumulated in
    ascending window index, so every canvas pixel sees acc = acc + p * v, ps = ps + p in the kernel's order, from 0."""
    n_w = len(ys) * len(xs)
    K = 0 if masks is None else int(np.asarray(masks).shape[1])
    e = np.asarray(eps, dtype=np.float32)
    C, h, w = e.shape[1:]
    e = e.reshape(K + 2, n_w, C, h, w)
    g = np.float32(g)
    Hc, Wc = canvas_hw
    acc, ps = np.zeros((C, Hc, Wc), dtype=np.float32), np.zeros((Hc, Wc), dtype=np.float32)
    p = (ramp_weights(h, ramp)[:, None] * ramp_weights(w, ramp)[None, :]).astype(np.float32)
    for iy, y0 in enumerate(ys):
        for ix, x0 in enumerate(xs):
            i = iy * len(xs) + ix
            if K:
                v = R.blend(e[:, i], np.asarray(masks, dtype=np.float32)[i:i + 1], np.asarray(weights, dtype=np.float32)[i:i + 1],
                            np.asarray(scales, dtype=np.float32)[i:i + 1], g)[0]
            else:
                u = e[1, i]
                v = u + g * (e[0, i] - u)
            acc[:, y0:y0 + h, x0:x0 + w] = acc[:, y0:y0 + h, x0:x0 + w] + p[None] * v
            ps[y0:y0 + h, x0:x0 + w] = ps[y0:y0 + h, x0:x0 + w] + p
    return acc / ps[None]


# ---- the loop fixture: the runner example's colours in bands over a wide map, the tiny UNet with 64-pixel windows

QK_GAIN = 4.0
STEPS = 8
GUIDANCE = 7.5
WINDOW, STRIDE = 64, 32                       # pixels: 8 and 4 latent pixels
PALETTE = list(cases.RUNNER_CONTEXT)
REGIONS = {(13, 255, 0): "an old oak tree with autumn leaves", (90, 206, 255): ("stormy sky with dark clouds", 0.8, 11.0)}
# name -> (map height, map width) in pixels, ramp, region prompts. "a" and "b" are the kernel cases of the same name; "e" is a canvas the
# tiny UNet also takes as ONE image (its three downsamplings need latent sides that are multiples of 8), which "a" and "b" are not: the
# plain whole-canvas call that the canvas result is held apart from exists only there.
LOOPS = {"a": ((64, 160), 0, None), "b": ((96, 88), 0, None), "e_ramp3": ((64, 192), 3, None), "a_regions": ((64, 160), 0, REGIONS)}
PLAIN = "e_ramp3"                              # the loop whose map the plain call also runs on
SEED = 3


def color_map(H, W):
    """Bands of the five colours, 24 pixels wide and 40 high, shifted by two colours per row of bands: edges fall inside the 8 x 8 blocks and
    inside the windows, and every 64-pixel window sees another mix of colours."""
    y, x = np.mgrid[0:H, 0:W]
    idx = (x // 24 + 2 * (y // 40)) % len(PALETTE)
    return np.ascontiguousarray(np.array(PALETTE, dtype=np.uint8)[idx])


def crops(rgb, ys, xs, h, w):
    return [np.ascontiguousarray(rgb[8 * y0:8 * (y0 + h), 8 * x0:8 * (x0 + w)]) for y0 in ys for x0 in xs]


def oracle_canvas_loop(name, steps=STEPS, seed=SEED, guidance=GUIDANCE, wf=cases.weight_fn_runner, qk_gain=QK_GAIN, plain=False):
    """fp32 CPU: the canvas loop over the oracle's pieces. Per window a cond / uncond dict (and region dicts) from the oracle's own
    encode_text_color_inputs on the window's crop of the map; the initial latent at canvas size; per step the windows of the scaled canvas
    latent through batch-1 UNet evaluations, `combine`, one scheduler step on the canvas. plain=True: the reference's loop on the whole map
    as one image, same seed."""
    (H, W), ramp, regions = LOOPS[name]
    vae, unet, text, tok, sch = cases.build_tools("tiny", qk_gain=qk_gain)
    rgb = color_map(H, W)
    O.install_oracle_attention(unet)
    try:
        if plain:
            return O.paint_with_words_latents(dict(cases.RUNNER_CONTEXT), rgb, cases.RUNNER_PROMPT, unet, text, tok, sch, num_inference_steps=steps,
                                              guidance_scale=guidance, seed=seed, weight_function=wf)
        h = w = WINDOW // 8
        ys, xs = grid(H // 8, W // 8, h, STRIDE // 8)
        zero = lambda w, sigma, qk: 0.0      # noqa: E731
        per = []                             # per window: [(dict, weight function)] in row-class order, base first, unconditional last
        masks = a = s = None
        if regions:
            colors, prompts, weights, scales = R.entries(regions, guidance)
            masks, a, s = [], [], []
        for crop in crops(rgb, ys, xs, h, w):
            _, _, cond, uncond = O.encode_text_color_inputs(text, tok, crop, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "")
            rows = [(cond, wf)]
            if regions:
                rows += [(O.encode_text_color_inputs(text, tok, crop, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, p)[3], zero) for p in prompts]
                masks.append(R.region_masks(crop, colors)), a.append(R.region_weights(weights, 0.0)), s.append(np.asarray(scales, dtype=np.float32))
            per.append(rows + [(uncond, zero)])
        extra_seeds, table, _, _ = O.encode_text_color_inputs(text, tok, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "")
        latents = O.initial_latents(seed, 4, H, W, table, extra_seeds)
        sch.set_timesteps(steps)
        latents = latents * sch.init_noise_sigma
        blend = {} if not regions else {"masks": np.stack(masks), "weights": np.stack(a), "scales": np.stack(s)}
        with torch.no_grad():
            for i, t in enumerate(sch.timesteps):
                sigma_t = sch.sigmas[i]
                x = sch.scale_model_input(latents, t)
                classes = [[] for _ in per[0]]
                for j, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
                    xw = x[:, :, y0:y0 + h, x0:x0 + w]
                    for cls, (d, f) in enumerate(per[j]):
                        d.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": f})
                        classes[cls].append(unet(xw, t, encoder_hidden_states=d).sample)
                eps = torch.cat([torch.cat(c) for c in classes]).numpy()
                noise = torch.from_numpy(combine(eps, ys, xs, (H // 8, W // 8), guidance, ramp, **blend))[None]
                latents = sch.step(noise, t, latents).prev_sample
        return latents
    finally:
        uninstall_all()


# ---- the recorded latents: tests/golden/canvas_oracle.npz (`python tests/canvas_cases.py` writes it); tests/test_canvas_host.py runs the
# loops again on the CPU and holds the record to them.
GOLDEN = os.path.join(cases.GOLDEN, "canvas_oracle.npz")
GOLDEN_TOL = 1e-4         # rel-L2 between two fp32 CPU runs of one loop (thread count and BLAS blocking change the summation order)
ORACLE_VISIBLE = 0.360    # CPU-measured rel-L2(canvas loop, plain whole-canvas loop) on PLAIN (profiles/canvas.md; the host test re-measures it)


def recorded():
    """name -> final latent [1, 4, Hc, Wc] of oracle_canvas_loop(name), and "plain": the whole-canvas loop on PLAIN's map."""
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in list(LOOPS) + ["plain"]}


if __name__ == "__main__":
    out = {name: oracle_canvas_loop(name).numpy() for name in LOOPS}
    out["plain"] = oracle_canvas_loop(PLAIN, plain=True).numpy()
    np.savez_compressed(GOLDEN, **out)
    d = out[PLAIN] - out["plain"]
    print("wrote", GOLDEN, "canvas vs plain on %s: rel-L2 %.3f" % (PLAIN, math.sqrt(float((d * d).sum()) / float((out["plain"] ** 2).sum()))))
