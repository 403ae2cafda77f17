#!/usr/bin/env python
"""What a canvas larger than the UNet's window costs (profiles/canvas.md).

1. The two launches of libpww_hip_canvas.so at the product shape -- a 64 x 256 latent canvas (512 x 2048 pixels), 64-pixel-latent windows every
   32: seven windows -- back to back, against the torch op sequence they replace: n_w slices + cat (+ the division, the cast and the
   replication for the row classes), ops.cfg_combine, n_w weighted adds and a divide.
2. One 512 x 2048 image, SD1.5 UNet topology, bf16, 30 PLMS steps, CFG 7.5, hipGraph mode, channels_last, MIOpen find mode:
     canvas   paint_with_words(canvas_window=512): seven windows, 14 rows per UNet evaluation, the two launches per step
     batch    paint_with_words_batch of seven 512 x 512 images (the crops under the windows, seeds 0 .. 6): the same rows without them
     plain    paint_with_words on the whole map as one image (N = 16384 in the first self-attention)
   `batch` and `plain` take code paths this feature does not touch, so they are what the parent commit runs. Alternating rounds; per
   setting one request that captures its graph if it has to, then the timed request that replays.

    python tools/time_canvas.py [--config sd15|tiny] [--steps 30] [--rounds 3] [--launches-only] [--skip-plain]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import pww_hip  # noqa: E402
import paint_with_words as pw  # noqa: E402
import pww_cases as cases  # noqa: E402
from pww_hip import ops  # noqa: E402

HC, WC, WIN, STRIDE = 64, 256, 64, 32


def torch_gather(canvas, ys, xs, h, w, denom, copies, dtype):
    rows = torch.cat([canvas[None, :, y0:y0 + h, x0:x0 + w] for y0 in ys for x0 in xs])
    return torch.cat([(rows / denom).to(dtype)] * copies)


def torch_combine(eps, ys, xs, hw, g):
    n_w = len(ys) * len(xs)
    v = ops.cfg_combine(eps[:n_w], eps[n_w:], g)
    h, w = v.shape[-2:]
    acc = torch.zeros((1, v.shape[1]) + tuple(hw), dtype=torch.float32, device=eps.device)
    ps = torch.zeros(hw, dtype=torch.float32, device=eps.device)
    for i, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
        acc[0, :, y0:y0 + h, x0:x0 + w] += v[i]
        ps[y0:y0 + h, x0:x0 + w] += 1.0
    return acc / ps


def stream_us(f, iters=200):
    for _ in range(10):
        f()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        f()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def time_launches(dev, dtype):
    ys, xs = ops.canvas_windows(HC, WIN, STRIDE), ops.canvas_windows(WC, WIN, STRIDE)
    g = torch.Generator().manual_seed(0)
    canvas = torch.randn(4, HC, WC, generator=g).to(dev)
    eps = torch.randn(2 * len(ys) * len(xs), 4, WIN, WIN, generator=g).to(dev, dtype)
    denom = 14.6
    pairs = {"gather": (lambda: ops.canvas_gather(canvas, ys, xs, WIN, WIN, denom, 2, dtype), lambda: torch_gather(canvas, ys, xs, WIN, WIN, denom, 2, dtype)),
             "combine": (lambda: ops.canvas_combine(eps, ys, xs, (HC, WC), 7.5), lambda: torch_combine(eps, ys, xs, (HC, WC), 7.5))}
    for name, (ours, theirs) in pairs.items():
        close = float((ours().float() - theirs().float()).abs().max())
        print("%s, %d windows of a %d x %d canvas, %s: pww_canvas_%s %.1f us, torch op sequence %.1f us (stream time per call, launch overhead "
              "included); max |difference| %.2e" % (name, len(ys) * len(xs), HC, WC, str(dtype)[6:], name, stream_us(ours), stream_us(theirs), close), flush=True)
    both = stream_us(lambda: (ops.canvas_gather(canvas, ys, xs, WIN, WIN, denom, 2, dtype), ops.canvas_combine(eps, ys, xs, (HC, WC), 7.5)))
    print("both launches back to back: %.1f us per step" % both, flush=True)


def wide_map(H=8 * HC, W=8 * WC):
    """The five colours of the runner example in bands, as wide as the canvas."""
    palette = np.array(list(cases.RUNNER_CONTEXT), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(palette[(x // 192 + 2 * (y // 320)) % len(palette)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches-only", action="store_true")
    ap.add_argument("--skip-plain", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    time_launches(dev, torch.bfloat16)
    if a.launches_only:
        return
    pww_hip.enable_miopen_find()
    tools = cases.build_tools(a.config, dtype=torch.bfloat16, device=dev, scheduler="plms")
    tools[1].to(memory_format=torch.channels_last)
    rgb = wide_map()
    xs = ops.canvas_windows(WC, WIN, STRIDE)
    crops = [Image.fromarray(np.ascontiguousarray(rgb[:, 8 * x0:8 * (x0 + WIN)])) for x0 in xs]
    kw = dict(num_inference_steps=a.steps, guidance_scale=7.5, device=dev, weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True)
    calls = {"canvas": lambda: pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=cases.RUNNER_PROMPT,
                                                   seed=0, canvas_window=8 * WIN, canvas_stride=8 * STRIDE, **kw),
             "batch": lambda: pw.paint_with_words_batch(dict(cases.RUNNER_CONTEXT), crops, cases.RUNNER_PROMPT, list(range(len(crops))), **kw)}
    if not a.skip_plain:
        calls["plain"] = lambda: pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=cases.RUNNER_PROMPT,
                                                     seed=0, **kw)

    def run(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calls[name]()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name in calls:
        run(name)                  # warm-up: MIOpen find at this shape, graph capture
    times = {name: [] for name in calls}
    for i in range(a.rounds):
        for name in calls:
            run(name)              # captures again where the previous setting replaced the graph
            times[name].append(run(name))
        print("round %d: %s" % (i, ", ".join("%s %.1f ms" % (name, times[name][-1] * 1e3) for name in calls)), flush=True)
    med = {name: sorted(t)[len(t) // 2] * 1e3 for name, t in times.items()}
    for name in calls:
        print("%s: ms per 512 x 2048 image %s" % (name, ", ".join("%.1f" % (t * 1e3) for t in sorted(times[name]))))
    print("canvas / batch of seven (medians): %.3f" % (med["canvas"] / med["batch"]))
    if "plain" in med:
        print("canvas / plain whole-canvas call (medians): %.3f" % (med["canvas"] / med["plain"]))


if __name__ == "__main__":
    main()
