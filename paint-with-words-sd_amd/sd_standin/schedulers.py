"""Scheduler stand-ins (diffusers==0.10.0 is pinned by the reference but not installable here).

``LMSDiscreteScheduler`` is the scheduler every reference entry point defaults to
(paint_with_words/paint_with_words.py:130, :400) and the only one its loop can run: the loop reads
``scheduler.sigmas[step_index]`` with ``step_index = (timesteps == t).nonzero().item()``
(:473-474). The published K-LMS algorithm is restated here: scaled-linear betas,
``sigma = sqrt((1 - abar) / abar)`` interpolated at ``linspace(0, T-1, n)[::-1]``, order-4 linear
multistep coefficients by numerical integration (scipy ``quad``, epsrel 1e-4).

``PLMSScheduler`` is the PNDM/PLMS scheduler (``skip_prk_steps=True``, ``steps_offset=1``: the SD
configuration) that BASELINE.json's headline config names. The reference cannot run it
(SURVEY.md section 8 a-note: no ``.sigmas`` and a repeated timestep), so its PwW sigma is DEFINED
here as ``sigma_t = sqrt((1 - abar_t) / abar_t)`` at the step's timestep and the step index is the
loop counter (``sigmas[i]`` / ``timesteps[i]``), which this class exposes with the same attribute
names so the same sampling loop drives both.
"""
from types import SimpleNamespace

import numpy as np
import torch
from scipy import integrate


def _scaled_linear_alphas_cumprod(beta_start, beta_end, num_train_timesteps):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class _Config(dict):
    """dict with attribute access (the reference calls ``scheduler.config.get("steps_offset", 0)``, :435)."""
    __getattr__ = dict.get


class LMSDiscreteScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear"):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError("stand-in implements the scaled_linear schedule SD uses")
        self.config = _Config(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                              beta_schedule=beta_schedule)
        self.alphas_cumprod = _scaled_linear_alphas_cumprod(beta_start, beta_end, num_train_timesteps)
        sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sigmas = np.concatenate([sigmas[::-1], [0.0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sigmas)
        self.init_noise_sigma = self.sigmas.max()
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=float)[::-1].copy())
        self.derivatives = []
        self._coeff_cache = {}

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        timesteps = np.linspace(0, self.config["num_train_timesteps"] - 1, num_inference_steps, dtype=float)[::-1].copy()
        sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sigmas)
        self.timesteps = torch.from_numpy(timesteps)
        if device is not None:
            self.sigmas = self.sigmas.to(device)
            self.timesteps = self.timesteps.to(device)
        self.derivatives = []
        self._coeff_cache = {}

    def _index(self, timestep):
        if torch.is_tensor(timestep):
            timestep = timestep.to(self.timesteps.device)
        return int((self.timesteps == timestep).nonzero().item())

    def scale_model_input(self, sample, timestep):
        sigma = self.sigmas[self._index(timestep)]
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def get_lms_coefficient(self, order, t, current_order):
        key = (order, t, current_order)
        if key not in self._coeff_cache:
            def lms_derivative(tau):
                prod = 1.0
                for k in range(order):
                    if current_order == k:
                        continue
                    prod *= (tau - self.sigmas[t - k]) / (self.sigmas[t - current_order] - self.sigmas[t - k])
                return prod
            self._coeff_cache[key] = integrate.quad(lms_derivative, self.sigmas[t], self.sigmas[t + 1], epsrel=1e-4)[0]
        return self._coeff_cache[key]

    def step(self, model_output, timestep, sample, order=4):
        step_index = self._index(timestep)
        sigma = self.sigmas[step_index]
        pred_original_sample = sample - sigma * model_output           # epsilon prediction
        derivative = (sample - pred_original_sample) / sigma
        self.derivatives.append(derivative)
        if len(self.derivatives) > order:
            self.derivatives.pop(0)
        order = min(step_index + 1, order)
        coeffs = [self.get_lms_coefficient(order, step_index, o) for o in range(order)]
        prev_sample = sample + sum(c * d for c, d in zip(coeffs, reversed(self.derivatives)))
        return SimpleNamespace(prev_sample=prev_sample, pred_original_sample=pred_original_sample)

    def add_noise(self, original_samples, noise, timesteps):
        sigmas = self.sigmas.to(device=original_samples.device, dtype=original_samples.dtype)
        idx = [self._index(t) for t in timesteps]
        sigma = sigmas[idx].flatten()
        while sigma.dim() < original_samples.dim():
            sigma = sigma.unsqueeze(-1)
        return original_samples + noise * sigma

    def __len__(self):
        return self.config["num_train_timesteps"]


class PLMSScheduler:
    """PNDM with skip_prk_steps (pseudo linear multistep, Liu et al. 2022), SD settings."""
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 steps_offset=1):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError("stand-in implements the scaled_linear schedule SD uses")
        self.config = _Config(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                              beta_schedule=beta_schedule, steps_offset=steps_offset, skip_prk_steps=True)
        self.alphas_cumprod = _scaled_linear_alphas_cumprod(beta_start, beta_end, num_train_timesteps)
        self.final_alpha_cumprod = self.alphas_cumprod[0]        # set_alpha_to_one=False
        self.init_noise_sigma = torch.tensor(1.0)
        self.timesteps = None
        self.sigmas = None
        self.ets = []
        self.counter = 0
        self.cur_sample = None

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        self.step_ratio = self.config["num_train_timesteps"] // num_inference_steps
        base = (np.arange(0, num_inference_steps) * self.step_ratio).round() + self.config["steps_offset"]
        # the second-to-last timestep is visited twice (the PLMS warm-up evaluation)
        plms = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
        self.timesteps = torch.from_numpy(plms.astype(np.int64))
        ac = self.alphas_cumprod[self.timesteps]
        # PwW sigma of each step (defined here, see module docstring); trailing 0 mirrors LMS.sigmas
        self.sigmas = torch.cat([((1 - ac) / ac) ** 0.5, torch.zeros(1)]).to(torch.float32)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self.ets = []
        self.counter = 0
        self.cur_sample = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        b_prev = 1 - a_prev
        sample_coeff = (a_prev / a_t) ** 0.5
        denom = a_t * b_prev ** 0.5 + (a_t * b_t * a_prev) ** 0.5
        return float(sample_coeff) * sample - float((a_prev - a_t) / denom) * model_output

    def step(self, model_output, timestep, sample):
        timestep = int(timestep)
        prev_timestep = timestep - self.step_ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep = timestep
            timestep = timestep + self.step_ratio
        if len(self.ets) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(self.ets) == 1 and self.counter == 1:
            model_output = (model_output + self.ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            model_output = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            model_output = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4])
        prev_sample = self._get_prev_sample(sample, timestep, prev_timestep, model_output)
        self.counter += 1
        return SimpleNamespace(prev_sample=prev_sample)

    def __len__(self):
        return self.config["num_train_timesteps"]


# ---- Euler, Euler ancestral, DDIM and DPM-Solver++(2M): the published updates in plain torch ------------------------------------------------
# Each `step` is the update as its paper / k-diffusion / diffusers writes it. Scalars are Python floats (the float64 value of the stored fp32
# sigma or alpha-bar), so a float64 sample is stepped in float64 and a float32 one as the scalar rounded to float32.

def _karras_sigmas(sigma_min, sigma_max, n, rho=7.0):
    """Karras et al. 2022, eq. 5: n sigmas from sigma_max down to sigma_min, equidistant in sigma^(1 / rho)."""
    ramp = np.linspace(0, 1, n)
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def _sigma_to_t(sigmas, all_sigmas):
    """The (fractional) training timestep of each sigma: linear in log sigma between the two neighbours of the training schedule."""
    log_all = np.log(all_sigmas)
    return np.interp(np.log(sigmas), log_all, np.arange(len(all_sigmas), dtype=float))


class _StepScheduler:
    """What the four classes below share: the constructor keywords of diffusers, the training schedule, the timestep lookup."""
    order = 1
    _space = "sigma"            # "sigma": x = x0 + sigma eps, the UNet sees x / sqrt(sigma^2 + 1); "vp": x = sqrt(abar) x0 + sqrt(1 - abar) eps

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", prediction_type="epsilon", **more):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError("stand-in implements the scaled_linear schedule SD uses")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError("prediction_type must be epsilon or v_prediction (got %r)" % (prediction_type,))
        self.config = _Config(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                              prediction_type=prediction_type, **more)
        self.alphas_cumprod = _scaled_linear_alphas_cumprod(beta_start, beta_end, num_train_timesteps)
        self._all_sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy().astype(np.float64)
        self.num_inference_steps = None
        self.timesteps = None
        self.sigmas = None
        self.init_noise_sigma = torch.tensor(1.0)

    def _index(self, timestep):
        if torch.is_tensor(timestep):
            timestep = timestep.to(self.timesteps.device)
        return int((self.timesteps == timestep).nonzero().item())

    def _x0(self, model_output, sample, sigma):
        """The model's estimate of x0 from a sample x0 + sigma eps (sigma space)."""
        if self.config["prediction_type"] == "epsilon":
            return sample - sigma * model_output
        return model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + sample / (sigma ** 2 + 1)

    def _x0_vp(self, model_output, sample, abar):
        """The same from a sample sqrt(abar) x0 + sqrt(1 - abar) eps (VP space)."""
        if self.config["prediction_type"] == "epsilon":
            return (sample - (1 - abar) ** 0.5 * model_output) / abar ** 0.5
        return abar ** 0.5 * sample - (1 - abar) ** 0.5 * model_output

    def _noise_scales(self, timesteps):
        """(a, b) of add_noise per timestep, each a timestep of the current schedule."""
        out = []
        for t in timesteps:
            sigma = float(self.sigmas[self._index(t)])
            out.append((1.0, sigma) if self._space == "sigma" else ((1 / (sigma ** 2 + 1)) ** 0.5, sigma * (1 / (sigma ** 2 + 1)) ** 0.5))
        return out

    def add_noise(self, original_samples, noise, timesteps):
        """a x0 + b z: (1, sigma) in sigma space, (sqrt(abar), sqrt(1 - abar)) in VP space."""
        ab = torch.tensor(self._noise_scales(timesteps), dtype=original_samples.dtype, device=original_samples.device)
        a, b = ab[:, 0], ab[:, 1]
        while a.dim() < original_samples.dim():
            a, b = a.unsqueeze(-1), b.unsqueeze(-1)
        return a * original_samples + b * noise

    def scale_model_input(self, sample, timestep=None):
        if self._space == "vp":
            return sample
        sigma = float(self.sigmas[self._index(timestep)])
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def _draw(self, sample):
        return torch.randn(sample.shape, dtype=sample.dtype, device=sample.device)

    def __len__(self):
        return self.config["num_train_timesteps"]


class EulerDiscreteScheduler(_StepScheduler):
    """Euler steps of the probability-flow ODE in sigma space (Karras et al. 2022, algorithm 1 without churn; k-diffusion `sample_euler`)."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", prediction_type="epsilon",
                 use_karras_sigmas=False):
        super().__init__(num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, use_karras_sigmas=use_karras_sigmas)
        self.sigmas = torch.from_numpy(np.concatenate([self._all_sigmas[::-1], [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(np.arange(num_train_timesteps, dtype=float)[::-1].copy())
        self.init_noise_sigma = self.sigmas.max()

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        timesteps = np.linspace(0, self.config["num_train_timesteps"] - 1, num_inference_steps, dtype=float)[::-1].copy()
        sigmas = np.interp(timesteps, np.arange(len(self._all_sigmas)), self._all_sigmas)
        if self.config["use_karras_sigmas"]:
            sigmas = _karras_sigmas(sigmas[-1], sigmas[0], num_inference_steps)
            timesteps = _sigma_to_t(sigmas, self._all_sigmas)
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(timesteps)
        self.init_noise_sigma = self.sigmas.max()
        if device is not None:
            self.sigmas, self.timesteps = self.sigmas.to(device), self.timesteps.to(device)

    def step(self, model_output, timestep, sample):
        i = self._index(timestep)
        sigma, sigma_next = float(self.sigmas[i]), float(self.sigmas[i + 1])
        pred_original_sample = self._x0(model_output, sample, sigma)
        derivative = (sample - pred_original_sample) / sigma
        prev_sample = sample + derivative * (sigma_next - sigma)
        return SimpleNamespace(prev_sample=prev_sample, pred_original_sample=pred_original_sample)


class EulerAncestralDiscreteScheduler(EulerDiscreteScheduler):
    """Ancestral sampling with Euler steps (k-diffusion `sample_euler_ancestral`, eta = 1): a step down to sigma_down and fresh noise of
    sigma_up. One torch.randn per step, from the global generator."""

    def step(self, model_output, timestep, sample):
        i = self._index(timestep)
        sigma, sigma_next = float(self.sigmas[i]), float(self.sigmas[i + 1])
        pred_original_sample = self._x0(model_output, sample, sigma)
        sigma_up = min(sigma_next, (sigma_next ** 2 * (sigma ** 2 - sigma_next ** 2) / sigma ** 2) ** 0.5)
        sigma_down = (sigma_next ** 2 - sigma_up ** 2) ** 0.5
        derivative = (sample - pred_original_sample) / sigma
        prev_sample = sample + derivative * (sigma_down - sigma)
        prev_sample = prev_sample + self._draw(sample) * sigma_up
        return SimpleNamespace(prev_sample=prev_sample, pred_original_sample=pred_original_sample)


def _leading_timesteps(num_train_timesteps, num_inference_steps, steps_offset):
    step_ratio = num_train_timesteps // num_inference_steps
    return ((np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy() + steps_offset).astype(np.int64), step_ratio


class DDIMScheduler(_StepScheduler):
    """DDIM (Song et al. 2021, eq. 12) in VP space, SD settings (set_alpha_to_one=False, no clipping). `eta` is a constructor keyword: the
    sampling loop calls step(noise_pred, t, latents) with nothing else. eta > 0 draws one torch.randn per step from the global generator.
    `sigmas[i]` is DEFINED as sqrt((1 - abar_t) / abar_t) at step i's timestep, as PLMSScheduler defines it."""
    _space = "vp"

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", prediction_type="epsilon",
                 steps_offset=1, eta=0.0):
        super().__init__(num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, steps_offset=steps_offset, eta=eta)
        self.eta = float(eta)
        self.final_alpha_cumprod = self.alphas_cumprod[0]        # set_alpha_to_one=False
        self.step_ratio = None
        self._custom = False

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        """`timesteps`: a descending list of integer training timesteps to visit instead of the evenly spaced ones; a step then goes to the
        next entry of the list."""
        self._custom = timesteps is not None
        if self._custom:
            ts = np.asarray(list(timesteps), dtype=np.int64)
            if ts.ndim != 1 or len(ts) < 1 or np.any(np.diff(ts) >= 0) or ts[-1] < 0 or ts[0] >= self.config["num_train_timesteps"]:
                raise ValueError("timesteps must be descending integers inside the training schedule")
            num_inference_steps, self.step_ratio = len(ts), None
        else:
            ts, self.step_ratio = _leading_timesteps(self.config["num_train_timesteps"], num_inference_steps, self.config["steps_offset"])
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts)
        ac = self.alphas_cumprod[self.timesteps]
        self.sigmas = torch.cat([((1 - ac) / ac) ** 0.5, torch.zeros(1)]).to(torch.float32)
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def _prev_timestep(self, timestep):
        if not self._custom:
            return timestep - self.step_ratio
        i = self._index(timestep)
        return int(self.timesteps[i + 1]) if i + 1 < len(self.timesteps) else -1

    def _noise_scales(self, timesteps):
        return [(float(self.alphas_cumprod[int(t)]) ** 0.5, (1 - float(self.alphas_cumprod[int(t)])) ** 0.5) for t in timesteps]

    def step(self, model_output, timestep, sample):
        timestep = int(timestep)
        prev_timestep = self._prev_timestep(timestep)
        abar = float(self.alphas_cumprod[timestep])
        abar_prev = float(self.alphas_cumprod[prev_timestep]) if prev_timestep >= 0 else float(self.final_alpha_cumprod)
        pred_original_sample = self._x0_vp(model_output, sample, abar)
        if self.config["prediction_type"] == "epsilon":
            pred_epsilon = model_output
        else:
            pred_epsilon = abar ** 0.5 * model_output + (1 - abar) ** 0.5 * sample
        variance = (1 - abar_prev) / (1 - abar) * (1 - abar / abar_prev)
        std = self.eta * variance ** 0.5
        direction = (1 - abar_prev - std ** 2) ** 0.5 * pred_epsilon
        prev_sample = abar_prev ** 0.5 * pred_original_sample + direction
        if self.eta > 0:
            prev_sample = prev_sample + std * self._draw(sample)
        return SimpleNamespace(prev_sample=prev_sample, pred_original_sample=pred_original_sample)


class DPMSolverMultistepScheduler(_StepScheduler):
    """DPM-Solver++(2M) (Lu et al. 2022): the second-order multistep solver on the data prediction, midpoint form, first order on the first
    executed step and on the last step, which goes to sigma = 0 and returns the data prediction itself.
    Convention: VP space, as diffusers -- x = alpha x0 + sigma_t eps, `scale_model_input` is the identity and `init_noise_sigma` 1.
    `sigmas[i]` is DEFINED as sqrt((1 - abar_t) / abar_t) = sigma_t / alpha_t at step i's timestep, as PLMSScheduler defines it; alpha_t and
    sigma_t of a step are formed from it. use_karras_sigmas: the sigmas are Karras's (rho = 7) between the smallest and largest sigma of the
    training schedule and the timesteps their fractional positions in it."""
    _space = "vp"

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", prediction_type="epsilon",
                 steps_offset=1, use_karras_sigmas=False, solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint"):
        if solver_order != 2 or algorithm_type != "dpmsolver++" or solver_type != "midpoint":
            raise NotImplementedError("stand-in implements DPM-Solver++(2M), midpoint")
        super().__init__(num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, steps_offset=steps_offset,
                         use_karras_sigmas=use_karras_sigmas, solver_order=solver_order, algorithm_type=algorithm_type, solver_type=solver_type)
        self.model_outputs = []

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        if self.config["use_karras_sigmas"]:
            sigmas = _karras_sigmas(self._all_sigmas[0], self._all_sigmas[-1], num_inference_steps)
            self.timesteps = torch.from_numpy(_sigma_to_t(sigmas, self._all_sigmas))
        else:
            ts, _ = _leading_timesteps(self.config["num_train_timesteps"], num_inference_steps, self.config["steps_offset"])
            sigmas = self._all_sigmas[ts]
            self.timesteps = torch.from_numpy(ts)
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self.model_outputs = []

    def step(self, model_output, timestep, sample):
        i = self._index(timestep)
        s, s_next = float(self.sigmas[i]), float(self.sigmas[i + 1])            # sigma_t / alpha_t of this step and of the next
        alpha, alpha_next = (1 / (s ** 2 + 1)) ** 0.5, (1 / (s_next ** 2 + 1)) ** 0.5
        x0 = self._x0_vp(model_output, sample, alpha ** 2)
        if s_next == 0.0:
            prev_sample = x0 * 1.0                                               # h is infinite: (sigma_next / sigma_t) = 0, -alpha expm1(-h) = 1
        else:
            h = float(np.log(s / s_next))                                        # lambda_next - lambda, lambda = log(alpha / sigma_t)
            ratio, gain = (s_next * alpha_next) / (s * alpha), -alpha_next * float(np.expm1(-h))
            if not self.model_outputs:
                prev_sample = ratio * sample + gain * x0
            else:
                s_last, x0_last = self.model_outputs[-1]
                r0 = float(np.log(s_last / s)) / h
                prev_sample = ratio * sample + gain * x0 + 0.5 * gain * ((x0 - x0_last) / r0)
        self.model_outputs = [(s, x0)]
        return SimpleNamespace(prev_sample=prev_sample, pred_original_sample=x0)
