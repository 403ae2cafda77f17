"""Cases and float64 restatements for the step plans (pww_hip/steps.py) and the step kernel (ops.sched_step).

The model of the host tests is the exact denoiser of Gaussian data x0 ~ N(0, S^2): with x = x0 + sigma eps, E[x0 | x] = x S^2 / (S^2 + sigma^2).
Its probability-flow solution is known in closed form, x(sigma) = x(sigma_0) sqrt((S^2 + sigma^2) / (S^2 + sigma_0^2)), which is what the
order-of-convergence test measures against. The published updates are written out directly here (k-diffusion's sample_euler,
sample_euler_ancestral and sample_dpmpp_2m in sigma space; DDIM's eq. 12 in VP space), independent of pww_hip.steps and of the scheduler
classes' step()."""
import math

import numpy as np
import torch

S = 0.7                       # standard deviation of the data
BETAS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
KINDS = ("euler", "euler_a", "ddim", "ddim_eta1", "dpmpp_2m")
PREDICTIONS = ("epsilon", "v_prediction")
SIGMA_SPACE = ("euler", "euler_a")
SHAPE = (1, 4, 4, 4)


def karras_integer_timesteps(sch, T):
    """DDIM has no Karras switch: the integer training timesteps nearest to Karras's sigmas (rho = 7), duplicates dropped."""
    from sd_standin.schedulers import _karras_sigmas, _sigma_to_t
    sig = _karras_sigmas(sch._all_sigmas[0], sch._all_sigmas[-1], T)
    ts = np.unique(np.rint(_sigma_to_t(sig, sch._all_sigmas)).astype(np.int64))[::-1]
    return [int(t) for t in ts]


def make(kind, prediction="epsilon", karras=False, T=None, **kw):
    """The scheduler of a case with SD's betas; with T its schedule is set."""
    from sd_standin import EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, DDIMScheduler, DPMSolverMultistepScheduler
    if kind in ("ddim", "ddim_eta1"):
        sch = DDIMScheduler(prediction_type=prediction, eta=1.0 if kind == "ddim_eta1" else 0.0, **dict(BETAS, **kw))
        if T is not None:
            sch.set_timesteps(timesteps=karras_integer_timesteps(sch, T)) if karras else sch.set_timesteps(T)
        return sch
    cls = {"euler": EulerDiscreteScheduler, "euler_a": EulerAncestralDiscreteScheduler, "dpmpp_2m": DPMSolverMultistepScheduler}[kind]
    sch = cls(prediction_type=prediction, use_karras_sigmas=karras, **dict(BETAS, **kw))
    if T is not None:
        sch.set_timesteps(T)
    return sch


def model(x_vp, sigma, prediction):
    """The exact model output for Gaussian data at noise level sigma, from the UNet's input x_vp = (x0 + sigma eps) / sqrt(sigma^2 + 1)."""
    alpha = 1.0 / math.sqrt(sigma * sigma + 1.0)
    x = x_vp / alpha
    x0 = x * (S * S / (S * S + sigma * sigma))
    eps = (x - x0) / sigma
    return eps if prediction == "epsilon" else alpha * eps - sigma * alpha * x0


def denoised(x_vp, sigma, prediction):
    """x0 as a sampler recovers it from the model output (the textbook conversions, in VP terms)."""
    alpha = 1.0 / math.sqrt(sigma * sigma + 1.0)
    m = model(x_vp, sigma, prediction)
    if prediction == "epsilon":
        return (x_vp - sigma * alpha * m) / alpha
    return alpha * x_vp - sigma * alpha * m


def sigmas_of(sch, timesteps):
    """float64 sigma of every executed step, then the sigma the last one goes to."""
    idx = [int((sch.timesteps == t).nonzero().item()) for t in timesteps]
    return [float(sch.sigmas[i]) for i in idx] + [float(sch.sigmas[idx[-1] + 1])]


def noises(T, seed=7):
    """The noise tensors a stochastic scheduler's step() draws under torch.manual_seed(seed): one float64 torch.randn of SHAPE per step."""
    torch.manual_seed(seed)
    return [torch.randn(SHAPE, dtype=torch.float64) for _ in range(T)]


def start(kind, sigma0, seed=3):
    """A float64 sample at the first noise level, in the scheduler's own space."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(SHAPE, generator=g, dtype=torch.float64) * math.sqrt(S * S + sigma0 * sigma0)
    return x if kind in SIGMA_SPACE else x / math.sqrt(sigma0 * sigma0 + 1.0)


def run_rows(kind, rows, sig, x, prediction, zs=None):
    """The seven-number recurrence in float64 over `rows` ([n, 7]); sig: sigma per row."""
    h = torch.zeros_like(x)
    for k, (p, r, a, b, c, e, d) in enumerate(np.asarray(rows, dtype=np.float64)):
        s = sig[k]
        m = model(x / math.sqrt(s * s + 1.0) if kind in SIGMA_SPACE else x, s, prediction)
        q = p * x + r * m
        xn = a * x + b * q
        if c != 0.0:
            xn = xn + c * h
        if e != 0.0:
            xn = xn + e * zs[k]
        x, h = xn, q
    return x


def run_class(sch, timesteps, x, prediction, seed=7):
    """The scheduler's own step() in float64 over `timesteps`, its noise drawn from the global generator under `seed`."""
    sig = sigmas_of(sch, timesteps)
    torch.manual_seed(seed)
    for k, t in enumerate(timesteps):
        m = model(sch.scale_model_input(x, t), sig[k], prediction)
        x = sch.step(m, t, x).prev_sample
    return x


def run_direct(kind, sch, timesteps, x, prediction, zs=None):
    """The published update written out directly, in float64."""
    sig = sigmas_of(sch, timesteps)
    if kind in SIGMA_SPACE:
        for k in range(len(timesteps)):
            s, sn = sig[k], sig[k + 1]
            den = denoised(x / math.sqrt(s * s + 1.0), s, prediction)
            d = (x - den) / s
            if kind == "euler":                                   # k-diffusion sample_euler
                x = x + d * (sn - s)
            else:                                                 # k-diffusion sample_euler_ancestral (get_ancestral_step, eta = 1)
                up = min(sn, math.sqrt(sn ** 2 * (s ** 2 - sn ** 2) / s ** 2))
                down = math.sqrt(sn ** 2 - up ** 2)
                x = x + d * (down - s)
                if sn > 0:
                    x = x + zs[k] * up
        return x
    if kind == "dpmpp_2m":                                        # k-diffusion sample_dpmpp_2m, in sigma space: x_sigma = x_vp / alpha
        x = x * math.sqrt(sig[0] ** 2 + 1.0)
        old = None
        for k in range(len(timesteps)):
            s, sn = sig[k], sig[k + 1]
            den = denoised(x / math.sqrt(s * s + 1.0), s, prediction)
            if sn == 0:
                x = den
            else:
                t, tn = -math.log(s), -math.log(sn)
                h = tn - t
                if old is None:
                    x = (sn / s) * x - math.expm1(-h) * den
                else:
                    r = (t - (-math.log(sig[k - 1]))) / h
                    x = (sn / s) * x - math.expm1(-h) * ((1 + 1 / (2 * r)) * den - (1 / (2 * r)) * old)
            old = den
        return x / math.sqrt(sig[-1] ** 2 + 1.0)
    eta = 1.0 if kind == "ddim_eta1" else 0.0                     # DDIM, Song et al. 2021, eq. 12
    for k, t in enumerate(timesteps):
        t = int(t)
        prev = sch._prev_timestep(t)
        ab = float(sch.alphas_cumprod[t])
        abn = float(sch.alphas_cumprod[prev]) if prev >= 0 else float(sch.final_alpha_cumprod)
        m = model(x, sig[k], prediction)          # (converted with the step's own abar: sigmas[] holds its fp32 rounding)
        x0 = (x - math.sqrt(1 - ab) * m) / math.sqrt(ab) if prediction == "epsilon" else math.sqrt(ab) * x - math.sqrt(1 - ab) * m
        eps =(x - math.sqrt(ab) * x0) / math.sqrt(1 - ab)
        std = eta * math.sqrt((1 - abn) / (1 - ab)) * math.sqrt(1 - ab / abn)
        x = math.sqrt(abn) * x0 + math.sqrt(1 - abn - std ** 2) * eps
        if eta:
            x = x + std * zs[k]
    return x


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def exact_flow(kind, x_start, sigma0, sigma_end):
    """The probability-flow solution at sigma_end of the sample x_start at sigma0, in the scheduler's own space."""
    to_sigma = (lambda x, s: x) if kind in SIGMA_SPACE else (lambda x, s: x * math.sqrt(s * s + 1.0))
    x = to_sigma(x_start, sigma0) * math.sqrt((S * S + sigma_end ** 2) / (S * S + sigma0 ** 2))
    return x if kind in SIGMA_SPACE else x / math.sqrt(sigma_end ** 2 + 1.0)


# ---- the kernel: a torch-CPU fp32 restatement in the header's order (include/pww_hip_step.h) ------------------------------------------------

def step_reference(x, row, model_out, g=0.0, h=None, z=None, out_dtype=None, copies=1):
    """-> (x', q, u or None), every operation one fp32 operation on CPU tensors. model_out: a (cond, uncond) pair of float16 / bfloat16
    tensors, or one fp32 tensor."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)      # noqa: E731
    p, r, a, b, c, e, d = (f(v) for v in row)
    if isinstance(model_out, tuple):
        cond, uncond = model_out[0].float(), model_out[1].float()
        m = uncond + f(g) * (cond - uncond)
    else:
        m = model_out
    q = (p * x) + (r * m)
    xn = (a * x) + (b * q)
    if float(c) != 0.0:
        xn = xn + (c * h)
    if float(e) != 0.0:
        xn = xn + (e * z)
    u = None
    if out_dtype is not None:
        u = torch.cat([(xn / d).to(out_dtype)] * copies, dim=0)
    return xn, q, u
