"""Step plans: Euler, Euler ancestral, DDIM and DPM-Solver++(2M) as ONE elementwise launch per step (ops.sched_step, libpww_hip_step.so).

Every one of these schedulers is the same affine update with different scalars. With x the fp32 latent, m the guided model output, h the
previous step's q and z a unit Gaussian:

    q  = p x + r m                      the step's estimate of x0
    x' = a x + b q [+ c h] [+ e z]      c = 0: the first executed step and the one-step methods; e = 0: a deterministic step
    h  = q
    u  = x' / d'                        the next UNet input; d' is what scale_model_input divides by at the NEXT timestep

so a scheduler is a table of seven numbers (p, r, a, b, c, e, d') per executed step, formed here on the host in float64 from the scheduler's
`sigmas` / `alphas_cumprod` and rounded once to fp32 (`plan`). The sampler (pww_hip/sampler.py) builds the plan once per request, keeps h
itself and issues one launch per step where it otherwise issues ops.cfg_combine, scheduler.step, the next step's scale_model_input, the cat
over the row classes and the cast; the scheduler object's own state is not advanced.

`covers(scheduler)` recognises a scheduler by class name plus config, the way pww_hip.vae.covers recognises a layout: the four classes of
sd_standin.schedulers, and a diffusers object of the same name and config by layout only. LMS and PLMS are NOT covered -- LMS needs four
history tensors, PLMS has a warm-up step that returns to a saved sample -- and keep the route of before, launch for launch.

PWW_STEP: "1" the fused launch where it is covered and the request allows it (the default, per scheduler: DEFAULTS below follow the
measurement of profiles/schedulers.md), "0" scheduler.step everywhere, "force" a decline is an error. A decline is a request of a scheduler
with one of the four names that cannot take the launch: a config this module does not know, a latent that is not float32, a missing library.
"""
import math
import os

import numpy as np
import torch

from . import ops
from . import _lib

SIGMA_SPACE = ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler")
NAMES = SIGMA_SPACE + ("DDIMScheduler", "DPMSolverMultistepScheduler")
# Per scheduler: is the fused launch the default? It is where tools/time_steps.py shows the gap between two graph replays no longer on the
# fused launch than on the stock sequence (profiles/schedulers.md, section 1).
DEFAULTS = {name: "1" for name in NAMES}

_STATS = {"requests": 0, "declined": 0}
_REASONS = {}


def mode(scheduler=None):
    """PWW_STEP: "0" | "1" | "force"; unset: the scheduler's entry of DEFAULTS."""
    v = os.environ.get("PWW_STEP")
    if v is None:
        return DEFAULTS.get(type(scheduler).__name__, "1")
    if v not in ("0", "1", "force"):
        raise ValueError("PWW_STEP must be 0, 1 or force (got %r)" % v)
    return v


def stats():
    """Since the last reset_stats(): fused_launches (launches of the step kernel), requests (requests that took the fused route), declined
    (+ decline_reasons: {reason: count}: requests of a scheduler with a covered name that kept scheduler.step)."""
    out = dict(_STATS)
    out["fused_launches"] = ops.STEP_LAUNCHES[0]
    out["decline_reasons"] = dict(_REASONS)
    return out


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0
    _REASONS.clear()
    ops.STEP_LAUNCHES[0] = 0


def _cfg(scheduler, key, default=None):
    config = getattr(scheduler, "config", None)
    if config is None:
        return default
    v = config.get(key, default) if hasattr(config, "get") else getattr(config, key, default)
    return default if v is None else v


def why_not(scheduler):
    """None if `plan` knows the scheduler, else the reason (a sentence); "" for a class of another name."""
    name = type(scheduler).__name__
    if name not in NAMES:
        return ""
    if _cfg(scheduler, "prediction_type", "epsilon") not in ("epsilon", "v_prediction"):
        return "prediction_type %r" % (_cfg(scheduler, "prediction_type"),)
    if _cfg(scheduler, "thresholding", False) or (name == "DDIMScheduler" and _cfg(scheduler, "clip_sample", False)):
        return "thresholding / clip_sample"
    if not hasattr(scheduler, "sigmas") or not hasattr(scheduler, "timesteps"):
        return "no sigmas / timesteps"
    if name == "DDIMScheduler" and not (hasattr(scheduler, "alphas_cumprod") and hasattr(scheduler, "final_alpha_cumprod")):
        return "no alphas_cumprod / final_alpha_cumprod"
    if name == "DPMSolverMultistepScheduler":
        if _cfg(scheduler, "solver_order", 2) != 2:
            return "solver_order %r" % (_cfg(scheduler, "solver_order"),)
        if _cfg(scheduler, "algorithm_type", "dpmsolver++") != "dpmsolver++":
            return "algorithm_type %r" % (_cfg(scheduler, "algorithm_type"),)
        if _cfg(scheduler, "solver_type", "midpoint") != "midpoint":
            return "solver_type %r" % (_cfg(scheduler, "solver_type"),)
    return None


def covers(scheduler):
    """Does `plan` know this scheduler? One of the four class names with a config it restates; False for LMS, PLMS and anything else."""
    return why_not(scheduler) is None


def stochastic(scheduler):
    """Does every step of the scheduler draw one noise tensor (Euler ancestral; DDIM with eta > 0)?"""
    name = type(scheduler).__name__
    return name == "EulerAncestralDiscreteScheduler" or (name == "DDIMScheduler" and float(getattr(scheduler, "eta", 0.0) or 0.0) > 0.0)


def _f64(v):
    return float(v.item()) if torch.is_tensor(v) else float(v)


def _index(scheduler, t):
    ts = scheduler.timesteps
    hits = (ts == (t.to(ts.device) if torch.is_tensor(t) else t)).nonzero()
    if hits.numel() != 1:
        raise ValueError("steps.plan: timestep %s is not exactly one entry of the scheduler's schedule" % _f64(t))
    return int(hits.item())


def rows64(scheduler, timesteps):
    """The table in float64: an array [len(timesteps), 7] of (p, r, a, b, c, e, d'), one row per EXECUTED step. `timesteps` are entries of
    scheduler.timesteps in the order they are run -- the whole schedule, or the suffix an img2img request runs: the first executed step has
    c = 0 whatever its index in the full schedule."""
    reason = why_not(scheduler)
    if reason is not None:
        raise ValueError("steps.plan: %s is not covered%s" % (type(scheduler).__name__, ": " + reason if reason else ""))
    name = type(scheduler).__name__
    v_pred = _cfg(scheduler, "prediction_type", "epsilon") == "v_prediction"
    idx = [_index(scheduler, t) for t in timesteps]
    sig = [_f64(s) for s in scheduler.sigmas]
    rows = np.zeros((len(idx), 7), dtype=np.float64)
    for k, i in enumerate(idx):
        s, s_next = sig[i], sig[i + 1]
        c = e = 0.0
        d = 1.0
        if name in SIGMA_SPACE:
            p, r = (1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0)) if v_pred else (1.0, -s)
            down = s_next
            if name == "EulerAncestralDiscreteScheduler":
                e = min(s_next, math.sqrt(s_next ** 2 * (s ** 2 - s_next ** 2) / s ** 2))
                down = math.sqrt(s_next ** 2 - e ** 2)
            a, b = down / s, 1.0 - down / s
            if k + 1 < len(idx):
                d = math.sqrt(sig[idx[k + 1]] ** 2 + 1.0)
        elif name == "DDIMScheduler":
            t = int(_f64(timesteps[k]))
            if hasattr(scheduler, "_prev_timestep"):
                prev = scheduler._prev_timestep(t)
            else:
                prev = t - int(_cfg(scheduler, "num_train_timesteps", 1000)) // int(scheduler.num_inference_steps)
            ab = _f64(scheduler.alphas_cumprod[t])
            ab_next = _f64(scheduler.alphas_cumprod[prev]) if prev >= 0 else _f64(scheduler.final_alpha_cumprod)
            eta = float(getattr(scheduler, "eta", 0.0) or 0.0)
            e = eta * math.sqrt((1.0 - ab_next) / (1.0 - ab) * (1.0 - ab / ab_next))
            p, r = (math.sqrt(ab), -math.sqrt(1.0 - ab)) if v_pred else (1.0 / math.sqrt(ab), -math.sqrt(1.0 - ab) / math.sqrt(ab))
            a = math.sqrt(1.0 - ab_next - e * e) / math.sqrt(1.0 - ab)
            b = math.sqrt(ab_next) - a * math.sqrt(ab)
        else:       # DPM-Solver++(2M) in VP space: the sigma-space table multiplied through by alpha
            alpha, alpha_next = 1.0 / math.sqrt(s * s + 1.0), 1.0 / math.sqrt(s_next * s_next + 1.0)
            p, r = (alpha, -s * alpha) if v_pred else (1.0 / alpha, -s)
            if s_next == 0.0:
                a, b = 0.0, 1.0
            else:
                h = math.log(s / s_next)
                gain = -alpha_next * math.expm1(-h)
                a, b = (s_next * alpha_next) / (s * alpha), gain
                if k > 0:
                    r0 = math.log(sig[idx[k - 1]] / s) / h
                    b, c = gain * (1.0 + 0.5 / r0), -0.5 * gain / r0
        rows[k] = (p, r, a, b, c, e, d)
    return rows


def plan(scheduler, timesteps):
    """One row (p, r, a, b, c, e, d') per EXECUTED step: rows64 rounded once to fp32, as a list of tuples of Python floats that are exact
    fp32 values (they travel in the kernel arguments of ops.sched_step)."""
    return [tuple(float(v) for v in row) for row in rows64(scheduler, timesteps).astype(np.float32)]


def route(scheduler, latents):
    """The sampler's decision for one request -> True: the fused launch; False: scheduler.step, as before. Counts a decline (and raises it
    under PWW_STEP=force) where a scheduler with one of the four names cannot take the launch."""
    reason = why_not(scheduler)
    if reason == "":
        return False            # LMS, PLMS, anything else: not this module's
    m = mode(scheduler)
    if m == "0":
        return False
    if reason is None and latents.dtype != torch.float32:
        reason = "the latent is %s, not float32" % latents.dtype
    if reason is None and not latents.is_cuda:
        reason = "the latent is not on a HIP device"
    if reason is None and _lib.load_step() is None:
        reason = "libpww_hip_step.so is missing"
    if reason is None:
        _STATS["requests"] += 1
        return True
    _STATS["declined"] += 1
    _REASONS[reason] = _REASONS.get(reason, 0) + 1
    if m == "force":
        raise _lib.PwwHipError("PWW_STEP=force: %s cannot take the fused step launch: %s" % (type(scheduler).__name__, reason))
    return False
