"""The region-strength fixture shared by tests/test_hold_host.py and tests/test_hold_gpu.py (test infrastructure): numpy fp32 restatements of
the three launches of libpww_hip_hold.so (include/pww_hip_hold.h) with the same operation order, the release rule restated, the kernel cases,
and the fp32 CPU img2img loop with a hold built from the oracle's pieces that both files compare against. Nothing in here calls the code
under test."""
import math
import os

import numpy as np
import torch

import canvas_cases as C
import pww_cases as cases
import region_prompt_cases as R
from gpu_util import uninstall_all
from oracle import pww_oracle as O

# the project's loop bars: rel-L2 of the final latent against the fp32 oracle loop, and against the unfused torch path's own drift
CAP = C.CAP
UNFUSED_SLACK = C.UNFUSED_SLACK


# ---- the release rule (the issue's definition, restated with numpy scalars)

def thresholds(T):
    """theta_g = fp32((T - g) / T), g = 0 .. T, the quotient in double."""
    return [np.float32(np.float64(T - g) / np.float64(T)) for g in range(T + 1)]


def first(T, s):
    """The smallest g with fp32(s) >= theta_g."""
    s = np.float32(s)
    return min(g for g, th in enumerate(thresholds(T)) if s >= th)


def reference_first(T, s):
    """The reference's img2img offset (paint_with_words.py:434-441 with steps_offset 0): T - min(int(T s), T), the product in double."""
    return T - min(int(T * s), T)


STEP_COUNTS = (1, 2, 3, 4, 5, 8, 10, 12, 15, 20, 25, 30, 40, 50, 100)
DISAGREE = ((50, 0.58), (100, 0.29), (100, 0.57), (100, 0.58))      # the reference's double product lands one ulp under an integer


def grid_pairs():
    """The (T, s) pairs of the 0.01, 0.05 and k / T grids, each once."""
    pairs = set()
    for T in STEP_COUNTS:
        for k in range(101):
            pairs.add((T, k / 100))
        for k in range(21):
            pairs.add((T, k * 0.05))
        for k in range(T + 1):
            pairs.add((T, k / T))
    return sorted(pairs)


# ---- numpy restatements (fp32, one operation at a time, in the header's order)

def strength_map(rgb, colors, strengths, s0, sigma=0.0):
    """pww_hold_strength_map (+ pww_hold_feather): S = ((s0 + m_1 d_1) + m_2 d_2) + ..., clamped, feathered."""
    base = np.float32(s0)
    m = R.box_masks(rgb, colors)                                   # [K, h, w], multiples of 1 / 64
    S = np.full(m.shape[1:], base, dtype=np.float32)
    for k, s in enumerate(strengths):
        d = np.float32(np.float32(s) - base)
        S = S + m[k] * d
    S = np.minimum(np.maximum(S, np.float32(0)), np.float32(1))
    return feather(S, sigma)


def feather(plane, sigma):
    """pww_hold_feather on one fp32 plane: the separable Gaussian of the region masks (rows, then columns), no plane limit."""
    return R.feather(np.asarray(plane, dtype=np.float32)[None], float(np.float32(sigma)))[0] if sigma > 0 else np.asarray(plane, dtype=np.float32)


def apply(x, x0, z, S, theta, a, b):
    """pww_hold_apply: x [n, C, ...], S [n, ...] numpy fp32 -> where(S < theta, a x0 + b z, x): two multiplications, one addition, a select."""
    a, b, theta = np.float32(a), np.float32(b), np.float32(theta)
    with np.errstate(invalid="ignore", over="ignore"):
        new = a * x0 + b * z
    return np.where((S < theta)[:, None], new, x).astype(np.float32)


# the kernel cases of hold_apply: (n, C, hw)
APPLY_CASES = ((1, 4, 64), (3, 4, 35), (2, 1, 64), (2, 4, 9216))
APPLY_AB = ((1.0, 14.6), (0.6, 0.8), (1.0, 0.0))
MAP_SIZES = ((64, 64), (72, 40), (70, 64))          # (H, W) of the colour map; 70: rows past 8 h are ignored
FEATHER_CASES = ((8, 8), (9, 5), (64, 256))         # 8 x 8: taps wider than the plane; 64 x 256: a canvas latent, larger than the masks' LDS plane
FEATHER_SIGMAS = (0.5, 2.0, 8.0)
COLORS8 = [(13, 255, 0), (90, 206, 255), (74, 18, 1), (0, 0, 0), (255, 255, 255), (1, 2, 3), (200, 100, 50), (7, 7, 7)]
STRENGTHS8 = [0.0, 1.0, 0.25, 0.9, 0.6, 0.1, 0.33, 0.75]


def apply_inputs(n, C, hw, seed=0):
    """x, x0, z, S for one hold_apply case: S on the 1 / 64 grid (so that S == k / 8 occurs), NaN and inf planted in x."""
    g = torch.Generator().manual_seed(seed + hw)
    x, x0, z = (torch.randn(n, C, hw, generator=g).numpy() for _ in range(3))
    S = (torch.randint(0, 65, (n, hw), generator=g).float() / 64).numpy()
    S[0, :9] = np.arange(9, dtype=np.float32) / 8                # every theta = k / 8 is met exactly
    x[0, 0, 0:3] = (np.nan, np.inf, -np.inf)                     # S = 0, 1/8, 2/8: held for theta above them ...
    x[0, C - 1, 6:9] = (np.nan, np.inf, -np.inf)                 # ... S = 6/8, 7/8, 1: released for theta at or below them
    return x, x0, z, S


def map_rgb(H, W, colors, seed=0, single=None):
    """A colour map of random rectangles in `colors` over a background that is none of them (edges fall inside the 8 x 8 blocks)."""
    rng = np.random.RandomState(seed + H + W)
    rgb = np.full((H, W, 3), 99, dtype=np.uint8)
    if single is not None:
        rgb[:] = single
        return rgb
    for _ in range(24):
        y0, x0 = rng.randint(0, H - 4), rng.randint(0, W - 4)
        rgb[y0:y0 + rng.randint(3, 30), x0:x0 + rng.randint(3, 30)] = colors[rng.randint(len(colors))]
    return rgb


# ---- the loop fixture: img2img on the tiny UNet, 8 steps, the LMS stand-in

QK_GAIN = C.QK_GAIN
STEPS = 8
GUIDANCE = 7.5
SEED = 5
PALETTE = C.PALETTE
A, B, D = PALETTE[0], PALETTE[1], PALETTE[2]


def _halves():
    rgb = np.zeros((64, 64, 3), dtype=np.uint8)
    rgb[:, :32] = A                     # the kept half: whole 8 x 8 blocks
    rgb[:40, 32:] = B
    rgb[40:, 32:] = D
    return rgb


def _stripes():
    rgb = np.zeros((64, 64, 3), dtype=np.uint8)
    rgb[:, :24], rgb[:, 24:40], rgb[:, 40:] = A, B, D
    return rgb


def _bands():
    rgb = np.zeros((64, 64, 3), dtype=np.uint8)
    rgb[:, :20], rgb[:, 20:44], rgb[:, 44:] = A, D, B      # edges inside the 8 x 8 blocks
    return rgb


# name -> (colour map, region_strength, strength (the base), feather, canvas?)
LOOPS = {
    "half_keep": (_halves, {A: 0.0}, 0.75, 0.0, False),
    "three": (_stripes, {A: 0.25, B: 0.5}, 1.0, 0.0, False),
    "feather2": (_bands, {A: 0.125, B: 0.875}, 0.5, 2.0, False),
    "canvas": (lambda: C.color_map(64, 160), {A: 0.0, B: 0.25}, 0.75, 0.0, True),
    "plain": (_halves, None, 0.75, 0.0, False),          # the plain img2img call on half_keep's map at its largest strength
}
WINDOW, STRIDE = C.WINDOW, C.STRIDE


def init_rgb(H, W):
    """The init image of a loop: smooth noise, uint8 [H, W, 3] (sides that are multiples of 32: `preprocess` does not resample)."""
    side = max(H, W)
    return np.ascontiguousarray(cases.synthetic_init_image(size=32 * ((side + 31) // 32), seed=83)[:H, :W])


def loop_inputs(name):
    make, region_strength, strength, sigma, canvas = LOOPS[name]
    rgb = make()
    return rgb, init_rgb(*rgb.shape[:2]), region_strength, strength, sigma, canvas


def oracle_hold_loop(name, steps=STEPS, seed=SEED, guidance=GUIDANCE, wf=cases.weight_fn_runner, qk_gain=QK_GAIN, trace=None):
    """fp32 CPU: the oracle's img2img loop with the hold restated behind every scheduler step. x0 from the VAE stand-in, z = randn after
    torch.manual_seed(seed), the first step from the release rule, (a, b) of the LMS stand-in's add_noise = (1, sigma of the step). The
    canvas loop evaluates the UNet per window as tests/canvas_cases.py::oracle_canvas_loop does. trace: a list that receives the latent
    behind every hold."""
    rgb, init, region_strength, strength, sigma, canvas = loop_inputs(name)
    H, W = rgb.shape[:2]
    vae, unet, text, tok, sch = cases.build_tools("tiny", qk_gain=qk_gain)
    O.install_oracle_attention(unet)
    try:
        zero = lambda w, sigma, qk: 0.0      # noqa: E731
        if canvas:
            h = w = WINDOW // 8
            ys, xs = C.grid(H // 8, W // 8, h, STRIDE // 8)
            per = [O.encode_text_color_inputs(text, tok, crop, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "")[2:] for crop in C.crops(rgb, ys, xs, h, w)]
        else:
            _, _, cond, uncond = O.encode_text_color_inputs(text, tok, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "")
        sch.set_timesteps(steps)
        x0 = 0.18215 * vae.encode(O._preprocess_rgb(init)).latent_dist.sample()
        torch.manual_seed(seed)
        z = torch.randn(x0.shape)
        theta = thresholds(steps)
        if region_strength is None:
            S, i0 = None, reference_first(steps, strength)
        else:
            S = strength_map(rgb, list(region_strength), list(region_strength.values()), strength, sigma)[None]
            i0 = first(steps, max([strength] + list(region_strength.values())))
        latents = sch.add_noise(x0, z, sch.timesteps[i0:i0 + 1])
        with torch.no_grad():
            for g in range(i0, steps):
                t, sigma_t = sch.timesteps[g], sch.sigmas[g]
                x = sch.scale_model_input(latents, t)
                if canvas:
                    classes = [[], []]
                    for j, (y0, x0_) in enumerate((y0, x0_) for y0 in ys for x0_ in xs):
                        xw = x[:, :, y0:y0 + h, x0_:x0_ + w]
                        for cls, (d, f) in enumerate(zip(per[j], (wf, zero))):
                            d.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": f})
                            classes[cls].append(unet(xw, t, encoder_hidden_states=d).sample)
                    eps = torch.cat([torch.cat(c) for c in classes]).numpy()
                    noise = torch.from_numpy(C.combine(eps, ys, xs, (H // 8, W // 8), guidance, 0))[None]
                else:
                    cond.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": wf})
                    eps_c = unet(x, t, encoder_hidden_states=cond).sample
                    uncond.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": zero})
                    eps_u = unet(x, t, encoder_hidden_states=uncond).sample
                    noise = O.cfg_combine(eps_c, eps_u, guidance)
                latents = sch.step(noise, t, latents).prev_sample
                if S is not None:
                    th, a, b = (theta[g + 1], 1.0, float(sch.sigmas[g + 1])) if g + 1 < steps else (theta[steps - 1], 1.0, 0.0)
                    latents = torch.from_numpy(apply(latents.numpy(), x0.numpy(), z.numpy(), S, th, a, b))
                    if trace is not None:
                        trace.append(latents.clone())
        return latents
    finally:
        uninstall_all()


def init_latent(name):
    """x0 of a loop, fp32 CPU."""
    vae = cases.build_tools("tiny")[0]
    return 0.18215 * vae.encode(O._preprocess_rgb(loop_inputs(name)[1])).latent_dist.sample()


# ---- the recorded latents: tests/golden/hold_oracle.npz (`python tests/hold_cases.py` writes it); tests/test_hold_host.py runs the loops
# again on the CPU and holds the record to them.
GOLDEN = os.path.join(cases.GOLDEN, "hold_oracle.npz")
GOLDEN_TOL = C.GOLDEN_TOL


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return math.sqrt(float(((a - b) ** 2).sum()) / float((b ** 2).sum()))


def recorded():
    """name -> final latent [1, 4, h, w] of oracle_hold_loop(name)."""
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in LOOPS}


if __name__ == "__main__":
    out = {name: oracle_hold_loop(name).numpy() for name in LOOPS}
    d = rel(out["plain"], out["half_keep"])
    print("plain vs half_keep: rel-L2 %.3f (must exceed %.3f)" % (d, 4 * max(CAP.values())))
    assert d > 4 * max(CAP.values()), "the fixture does not discriminate: choose a larger kept region"
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, {k: v.shape for k, v in out.items()})
