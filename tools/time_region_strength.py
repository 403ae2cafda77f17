"""Timing of region strength (profiles/region_strength.md): the hold launch against the torch sequence it replaces, the one-off strength map
and feather of a request, and a whole region-strength request against the plain img2img call of the same step count.

    python tools/time_region_strength.py [--pairs 4] [--steps 20] [--config sd15] [--skip-request]

Device timestamps (event pairs around a batch of launches), warmed up, medians over several batches with the spread printed beside them;
the two whole requests run in one process as alternating pairs."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
from PIL import Image


def device_us(fn, reps=200, batches=7, warm=50):
    """Median (and min .. max) over `batches` of the device time of one call, from an event pair around `reps` calls."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def show(name, t):
    print("%-58s %8.2f us  (%.2f .. %.2f)" % (name, t[0], t[1], t[2]), flush=True)


def time_launches(dev):
    from pww_hip import ops
    g = torch.Generator().manual_seed(0)
    for shape in ((1, 4, 64, 64), (1, 4, 64, 256)):
        x, x0, z = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
        S = torch.rand(shape[:1] + shape[2:], generator=g).to(dev)
        theta, a, b = 0.5, 1.0, 3.7
        tag = "x".join(map(str, shape))
        show("hold_apply %s (half of the pixels held)" % tag, device_us(lambda: ops.hold_apply(x, x0, z, S, theta, a, b)))
        show("hold_apply %s (nothing held)" % tag, device_us(lambda: ops.hold_apply(x, x0, z, S, 0.0, a, b)))
        show("torch.where(S < theta, a * x0 + b * z, x) %s" % tag, device_us(lambda: torch.where((S < theta)[:, None], a * x0 + b * z, x)))
        xl = x.contiguous(memory_format=torch.channels_last)
        show("channels_last latent %s: NCHW copy, hold_apply, copy back" % tag, device_us(lambda: xl.copy_(ops.hold_apply(xl.contiguous(), x0, z, S, theta, a, b))))
    import hold_cases as H
    for (Hh, W) in ((512, 512), (512, 2048)):
        rgb = torch.from_numpy(np.ascontiguousarray(np.array(H.COLORS8, dtype=np.uint8)[np.random.RandomState(0).randint(0, 8, (Hh // 4, W // 4))].repeat(4, 0).repeat(4, 1))).to(dev)
        tag = "%dx%d map" % (Hh, W)
        show("hold_strength_map %s, 8 colours" % tag, device_us(lambda: ops.hold_strength_map(rgb, H.COLORS8, H.STRENGTHS8, 0.5), reps=50))
        show("hold_strength_map %s, 8 colours + feather 2" % tag, device_us(lambda: ops.hold_strength_map(rgb, H.COLORS8, H.STRENGTHS8, 0.5, 2.0), reps=50))
        show("hold_strength_map %s, 8 colours + feather 8" % tag, device_us(lambda: ops.hold_strength_map(rgb, H.COLORS8, H.STRENGTHS8, 0.5, 8.0), reps=50))


def time_request(dev, config, steps, pairs):
    import paint_with_words as pw
    import pww_hip
    import pww_cases as cases
    import importlib
    pww_hip.enable_miopen_find()
    importlib.import_module("paint_with_words.paint_with_words").DEFAULT_MODE = "graph"
    tools = cases.build_tools(config, dtype=torch.bfloat16, device=dev)
    rgb = cases.load_example_rgb()
    init = Image.fromarray(np.ascontiguousarray(cases.synthetic_init_image(max(rgb.shape[:2]))[:rgb.shape[0], :rgb.shape[1]]))
    colors = list(cases.RUNNER_CONTEXT)
    strengths = {colors[0]: 0.0, colors[1]: 0.25, colors[2]: 0.75}

    def call(region):
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kw = dict(region_strength=strengths, region_strength_feather=2.0) if region else {}
        pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=cases.RUNNER_PROMPT,
                            num_inference_steps=steps, guidance_scale=7.5, device=str(dev), weight_function=cases.weight_fn_runner, preloaded_utils=tools,
                            return_latents=True, init_image=init, strength=0.75, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for region in (False, True, False, True):      # capture, MIOpen's search, the library load
        call(region)
    plain, held = [], []
    for _ in range(pairs):
        plain.append(call(False))
        held.append(call(True))
    n_steps = steps - (steps - int(steps * 0.75))
    print("whole request, %s bf16 graph mode, %d of %d steps, %d alternating pairs (ms)" % (config, n_steps, steps, pairs))
    print("  plain img2img     : %s  median %.1f  spread %.2f %%" % (" ".join("%.1f" % v for v in plain), statistics.median(plain), 100 * (max(plain) - min(plain)) / statistics.median(plain)))
    print("  region strength   : %s  median %.1f  spread %.2f %%" % (" ".join("%.1f" % v for v in held), statistics.median(held), 100 * (max(held) - min(held)) / statistics.median(held)))
    print("  ratio of the medians %.4f; per pair %s" % (statistics.median(held) / statistics.median(plain), " ".join("%.4f" % (h / p) for h, p in zip(held, plain))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--skip-request", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    time_launches(dev)
    if not args.skip_request:
        time_request(dev, args.config, args.steps, args.pairs)
