"""Timing of the fused sampler step (profiles/schedulers.md): (a) what lies between two graph replays -- the one ops.sched_step launch
against the stock sequence it replaces (ops.cfg_combine, scheduler.step, the next step's scale_model_input, the cat over the row classes, the
cast and the copy into the graph's static input) -- per scheduler at the SD1.5 latent, 2 rows; (b) whole 512 x 512 requests in hipGraph
mode: every sampler name fused against PWW_STEP=0, and dpmpp_2m at 20 steps and euler_a at 30 against PLMS at 30.

    python tools/time_steps.py [--pairs 5] [--config sd15] [--skip-request]

(a): device timestamps (an event pair around a batch of back-to-back sequences), warmed up, medians over several batches with the spread
beside them, A and B alternating batch by batch. (b): a host clock around a request that ends in a synchronise, alternating in one
process."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import torch
from PIL import Image

BETAS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)


def _batch_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternating_us(fa, fb, reps=200, batches=9, warm=50):
    """Medians (and min .. max) of two sequences, their batches alternating."""
    for _ in range(warm):
        fa(), fb()
    ta, tb = [], []
    for _ in range(batches):
        ta.append(_batch_us(fa, reps))
        tb.append(_batch_us(fb, reps))
    return tuple((statistics.median(t), min(t), max(t)) for t in (ta, tb))


def schedulers():
    from sd_standin import EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, DDIMScheduler, DPMSolverMultistepScheduler
    return {"euler": EulerDiscreteScheduler(**BETAS), "euler_a": EulerAncestralDiscreteScheduler(**BETAS), "ddim": DDIMScheduler(**BETAS),
            "ddim eta=1": DDIMScheduler(eta=1.0, **BETAS), "dpmpp_2m": DPMSolverMultistepScheduler(**BETAS),
            "dpmpp_2m_karras": DPMSolverMultistepScheduler(use_karras_sigmas=True, **BETAS)}


def time_gap(dev, dtype=torch.bfloat16, rows=2, T=20):
    from pww_hip import ops, steps
    g = torch.Generator().manual_seed(0)
    shape = (1, 4, 64, 64)
    eps = torch.randn((rows,) + shape[1:], generator=g).to(dev, dtype)
    eps_c, eps_u = eps[:1], eps[1:]
    static_in = torch.empty((rows,) + shape[1:], dtype=dtype, device=dev)
    print("between two replays, latent %s, %d rows, %s: median us (min .. max) of back-to-back sequences" % ("x".join(map(str, shape)), rows, dtype))
    for name, sch in schedulers().items():
        sch.set_timesteps(T)
        t0, t1, t2 = sch.timesteps[0], sch.timesteps[1], sch.timesteps[2]
        lat0 = (torch.randn(shape, generator=g) * float(sch.init_noise_sigma)).to(dev)
        sch.step(torch.zeros_like(lat0), t0, lat0)               # (DPM-Solver++: the history of the second step)
        row = steps.plan(sch, sch.timesteps)[1]
        x, h = lat0.clone(), torch.zeros_like(lat0)
        draws = steps.stochastic(sch)
        history = getattr(sch, "model_outputs", None)            # (every timed step is the schedule's second: its history is the first step's)

        def stock():
            if history is not None:
                sch.model_outputs = history
            noise = ops.cfg_combine(eps_c, eps_u, 7.5)
            lat = sch.step(noise, t1, lat0).prev_sample
            static_in.copy_(torch.cat([sch.scale_model_input(lat, t2)] * rows, dim=0).to(dtype))

        def fused():
            z = torch.randn(shape, dtype=torch.float32, device=dev) if draws else None
            ops.sched_step(x, row, (eps_c, eps_u), 7.5, h=h if row[4] != 0.0 else None, z=z, u=static_in)

        def kernel():
            ops.sched_step(x, row, (eps_c, eps_u), 7.5, h=h if row[4] != 0.0 else None, z=lat0 if draws else None, u=static_in)
        (a, b) = alternating_us(stock, fused)
        (k, _) = alternating_us(kernel, kernel, batches=5)
        print("  %-16s stock sequence %7.2f (%.2f .. %.2f)   fused launch %6.2f (%.2f .. %.2f)   kernel alone %6.2f   stock / fused %.2f"
              % (name, a[0], a[1], a[2], b[0], b[1], b[2], k[0], a[0] / b[0]), flush=True)


def time_requests(dev, config, pairs):
    import importlib
    import paint_with_words as pw
    import pww_hip
    import pww_cases as cases
    from pww_hip import steps
    pww_hip.enable_miopen_find()
    importlib.import_module("paint_with_words.paint_with_words").DEFAULT_MODE = "graph"
    tools = cases.build_tools(config, dtype=torch.bfloat16, device=dev, scheduler="plms")
    rgb = cases.load_example_rgb()

    def call(sampler, n_steps, env):
        os.environ["PWW_STEP"] = env
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=cases.RUNNER_PROMPT,
                            num_inference_steps=n_steps, guidance_scale=7.5, device=str(dev), weight_function=cases.weight_fn_runner, preloaded_utils=tools,
                            return_latents=True, **({} if sampler is None else {"sampler": sampler}))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    med = statistics.median
    spread = lambda v: 100 * (max(v) - min(v)) / med(v)      # noqa: E731
    for _ in range(2):                                       # capture, MIOpen's search, the library load
        call(None, 30, "1"), call("dpmpp_2m", 20, "1"), call("dpmpp_2m", 20, "0")
    print("whole request, %s bf16 %dx%d, hipGraph mode, %d alternating runs each (ms)" % (config, rgb.shape[1], rgb.shape[0], pairs))
    for name, n_steps in (("euler", 30), ("euler_a", 30), ("ddim", 30), ("dpmpp_2m", 20), ("dpmpp_2m_karras", 20)):
        call(name, n_steps, "1"), call(name, n_steps, "0")
        steps.reset_stats()
        plms, fused, stock = [], [], []
        for _ in range(pairs):
            plms.append(call(None, 30, "1"))
            fused.append(call(name, n_steps, "1"))
            stock.append(call(name, n_steps, "0"))
        assert steps.stats()["fused_launches"] == pairs * n_steps and steps.stats()["declined"] == 0
        print("  %-16s %2d steps: fused %7.1f (spread %.1f %%)  PWW_STEP=0 %7.1f (%.1f %%)  fused / stock %.4f | PLMS 30 steps %7.1f (%.1f %%)  fused / PLMS %.3f"
              % (name, n_steps, med(fused), spread(fused), med(stock), spread(stock), med(fused) / med(stock), med(plms), spread(plms), med(fused) / med(plms)),
              flush=True)
    os.environ.pop("PWW_STEP", None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--skip-request", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    time_gap(dev)
    if not args.skip_request:
        time_requests(dev, args.config, args.pairs)
