"""The LoRA fixtures shared by tests/test_lora_host.py and tests/test_lora_gpu.py (test infrastructure): random adapters in both key
grammars, the operands and the fp64 evaluation of one kernel case, and the fp32 CPU oracle loop in which every row class is evaluated by a
deep copy of the UNet with that class's adapter MERGED into its weights. Nothing in here calls the code under test."""
import copy
import os

import numpy as np
import torch

import pww_cases as cases
import region_prompt_cases as R
from gpu_util import uninstall_all
from negative_cases import CAP  # noqa: F401  (the loop caps: tests/test_loop_gpu.py::test_tiny_loop_vs_reference)
from oracle import pww_oracle as O

TARGETS = ("to_q", "to_k", "to_v", "to_out.0")


# ---- adapters
def attention_paths(unet):
    return [p for p, m in unet.named_modules() if m.__class__.__name__ == "CrossAttention"]


def _weight(unet, path, target):
    m = dict(unet.named_modules())[path]
    return (m.to_out[0] if target == "to_out.0" else getattr(m, target)).weight


def make_factors(unet, seed, rank=4, gain=1.0, alpha=None, targets=TARGETS, gain_qk=None):
    """{(attention module path, target): (down [rank, K], up [N, rank], alpha or None)} in fp32: down ~ N(0, 1 / K), up ~ N(0, gain^2 / rank),
    so that up @ down has entries of about gain / sqrt(K) -- the size of the base weights' own for gain = 1. gain_qk: another gain for
    to_q and to_k (the projections in front of the softmax), default the same."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for p in attention_paths(unet):
        for t in targets:
            N, K = _weight(unet, p, t).shape
            gt = gain_qk if gain_qk is not None and t in ("to_q", "to_k") else gain
            out[(p, t)] = (torch.randn(rank, K, generator=g) / K ** 0.5, torch.randn(N, rank, generator=g) * (gt / rank ** 0.5), alpha)
    return out


def kohya_dict(factors):
    d = {}
    for (p, t), (down, up, alpha) in factors.items():
        stem = "lora_unet_" + (p + "." + t).replace(".", "_")
        d[stem + ".lora_down.weight"], d[stem + ".lora_up.weight"] = down.clone(), up.clone()
        if alpha is not None:
            d[stem + ".alpha"] = torch.tensor(float(alpha))
    return d


def peft_dict(factors, prefix="unet."):
    d = {}
    for (p, t), (down, up, alpha) in factors.items():
        stem = prefix + p + "." + t
        d[stem + ".lora_A.weight"], d[stem + ".lora_B.weight"] = down.clone(), up.clone()
        if alpha is not None:
            d[stem + ".alpha"] = torch.tensor(float(alpha))
    return d


def merged(unet, factors, scale):
    """A deep copy of `unet` with W + scale * (alpha / rank) * up @ down in every projection of `factors`, formed in the weights' dtype's
    fp32 / fp64 arithmetic (the copy keeps the dtype)."""
    u = copy.deepcopy(unet)
    if factors is None or scale == 0:
        return u
    for (p, t), (down, up, alpha) in factors.items():
        w = _weight(u, p, t)
        rank = down.shape[0]
        a = rank if alpha is None else alpha
        with torch.no_grad():
            w.add_(((float(scale) * a / rank) * (up.double() @ down.double())).to(device=w.device, dtype=w.dtype))
    return u


# ---- one kernel case
class Rows:
    """The part of lora.LoraState that ops.lora_update reads."""

    def __init__(self, adapters, scales, device):
        self.row_adapter = torch.tensor(adapters, dtype=torch.int32, device=device)
        self.row_scale = torch.tensor(scales, dtype=torch.float32, device=device)

    def _ensure_rows(self):
        pass


ROW_ADAPTERS, ROW_SCALES = [-1, 0, 1, 0], [1.0, 1.0, -0.5, 0.0]
SENTINEL = 77.0


def kernel_case(T, K, N, n_seg, rank, dtype, device, seed=0):
    """Operands of one launch, R = 4: x = a [R, T, K] view of a buffer with token stride K + 8, y = the [R, T, N] view at column 8 of a
    [R, T + 3, N + 24] buffer filled with SENTINEL, two adapters (the second one of true rank 8, zero-padded), values of the storage type."""
    g = torch.Generator().manual_seed(seed + 1000 * T + K + N)
    Rr = len(ROW_ADAPTERS)
    xbuf = torch.full((Rr, T, K + 8), SENTINEL)
    xbuf[..., :K] = torch.randn(Rr, T, K, generator=g)
    ybuf = torch.full((Rr, T + 3, N + 24), SENTINEL)
    ybuf[:, :T, 8:8 + N] = torch.randn(Rr, T, N, generator=g)
    A = torch.randn(2, n_seg, rank, K, generator=g) / K ** 0.5
    B = torch.randn(2, n_seg, N // n_seg, rank, generator=g) / rank ** 0.5
    A[1, :, 8:], B[1, :, :, 8:] = 0, 0
    xbuf, ybuf, A, B = (t.to(device=device, dtype=dtype) for t in (xbuf, ybuf, A, B))
    return dict(xbuf=xbuf, ybuf=ybuf, x=xbuf[..., :K], y=ybuf[:, :T, 8:8 + N], A=A.contiguous(), B=B.contiguous(), n_seg=n_seg)


def kernel_exact(case, dtype):
    """fp64 evaluation of the header's formula on the case's storage-type values: t rounded once to the storage type (that is its
    definition), everything else exact. -> fp64 [R, T, N]."""
    x, y, A, B = (case[k].double().cpu() for k in ("x", "y", "A", "B"))
    out = y.clone()
    ns = y.shape[-1] // case["n_seg"]
    for r, (i, s) in enumerate(zip(ROW_ADAPTERS, ROW_SCALES)):
        if i < 0 or s == 0:
            continue
        for g in range(case["n_seg"]):
            t = (x[r] @ A[i, g].t()).to(dtype).double()
            out[r, :, g * ns:(g + 1) * ns] += s * (t @ B[i, g].t())
    return out


# ---- the oracle loop: every row class on its own merged copy of the fp32 CPU UNet
# Two adapters over every attention projection of the tiny UNet. "a": rank 4, alpha = rank. "b": rank 8 with alpha 4 (a factor 1 / 2).
# The gains are chosen so that the ORACLE's final latent moves by at least 10 x the loop cap of bf16 (10 x 0.1) -- measured on the CPU,
# tests/scripts/make_lora_golden.py prints the figures: rel-L2 global / without 1.300, regions / regions_without 2.145, swapped / regions 1.293
# (1.302 the other way round) -- while the loop stays as well conditioned as the adapter-free one: a 1e-4 relative perturbation of the
# initial latent moves the final latent by 7e-5 (1.1e-4 without adapters). That needs a small gain in front of the softmax: with the
# same gain 1.25 on all four projections the figures were 1.458 / 1.235 / 1.117, but the same perturbation moved the latent by 1.2e-2, and
# the half-precision loops -- the unfused torch ops as much as the kernels -- ended 7e-2 (fp16) and 0.27 (bf16) from the oracle.
ADAPTERS = {"a": dict(seed=11, rank=4, gain=4.0, gain_qk=0.25), "b": dict(seed=12, rank=8, gain=8.0, gain_qk=0.5, alpha=4.0)}
GLOBAL = ("a", 1.0)
# the two largest colours of the runner example's map (sky 49 %, ground 29 % of the pixels)
REGIONS2 = {c: R.REGIONS[c] for c in ((90, 206, 255), (74, 18, 1))}
REGION_LORAS = {(90, 206, 255): ("a", 1.0), (74, 18, 1): ("b", 1.0)}
SWAPPED_LORAS = {(90, 206, 255): ("b", 1.0), (74, 18, 1): ("a", 1.0)}
STEPS = R.STEPS


def adapter_factors(unet, name):
    return make_factors(unet, **ADAPTERS[name])


def oracle_loop(lora=None, regions=None, region_loras=None, steps=STEPS, seed=0, guidance=R.GUIDANCE, wf=cases.weight_fn_runner, config="tiny",
                qk_gain=R.QK_GAIN):
    """fp32 CPU: region_prompt_cases.oracle_loop with every row class evaluated by its own UNet -- a deep copy with the class's adapter
    merged in (W + scale * alpha / rank * up @ down). lora: (name, scale) for the base row, the unconditional row and regions without an
    entry; region_loras: {colour: (name, scale)}."""
    vae, unet, text, tok, sch = cases.build_tools(config, qk_gain=qk_gain)
    rgb = cases.load_example_rgb()
    copies = {}

    def unet_of(entry):
        if entry is None:
            return unet
        if entry not in copies:
            copies[entry] = merged(unet, adapter_factors(unet, entry[0]), entry[1])
        return copies[entry]
    O.install_oracle_attention(unet)
    try:
        extra_seeds, table, cond, uncond = O.encode_text_color_inputs(text, tok, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, "")
        zero = lambda w, sigma, qk: 0.0      # noqa: E731
        rdicts, runets = [], []
        if regions:
            colors, prompts, weights, scales = R.entries(regions, guidance)
            rdicts = [R.region_dict(text, tok, rgb, p) for p in prompts]
            runets = [unet_of((region_loras or {}).get(c, lora)) for c in colors]
            masks = R.region_masks(rgb, colors, 0.0)[None]
            a, s = R.region_weights(weights, 0.0)[None], np.asarray(scales, dtype=np.float32)[None]
        base = unet_of(lora)
        latents = O.initial_latents(seed, 4, rgb.shape[0], rgb.shape[1], table, extra_seeds)
        sch.set_timesteps(steps)
        latents = latents * sch.init_noise_sigma
        with torch.no_grad():
            for i, t in enumerate(sch.timesteps):
                sigma_t = sch.sigmas[i]
                x = sch.scale_model_input(latents, t)
                cond.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": wf})
                rows = [base(x, t, encoder_hidden_states=cond).sample]
                for d, u in zip(rdicts + [uncond], runets + [base]):
                    d.update({"SIGMA": sigma_t, "WEIGHT_FUNCTION": zero})
                    rows.append(u(x, t, encoder_hidden_states=d).sample)
                if rdicts:
                    noise = torch.from_numpy(R.blend(torch.cat(rows).numpy(), masks, a, s, guidance))
                else:
                    noise = O.cfg_combine(rows[0], rows[1], guidance)
                latents = sch.step(noise, t, latents).prev_sample
        return latents
    finally:
        uninstall_all()


# ---- the oracle loop's recorded latents (tests/scripts/make_lora_golden.py writes them; tests/test_lora_host.py re-runs one)
GOLDEN = os.path.join(cases.GOLDEN, "lora_oracle.npz")
RECORDED = {"without": dict(), "global": dict(lora=GLOBAL),
            "regions_without": dict(regions=REGIONS2), "regions": dict(regions=REGIONS2, region_loras=REGION_LORAS),
            "swapped": dict(regions=REGIONS2, region_loras=SWAPPED_LORAS)}


def recorded():
    """name -> final latent [1, 4, 64, 64] of oracle_loop(**RECORDED[name])."""
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in RECORDED}
