#!/usr/bin/env python
"""What a negative context costs end to end (profiles/negative_regions.md): BASELINE config 2's shape -- SD1.5 UNet topology, 512 x 512,
bf16, the 5-region example map, 30 PLMS steps, CFG 7.5, batch 1, hipGraph mode, channels_last, MIOpen find mode -- without a negative
context and with a 2-region one (tree and dog, named in the unconditional prompt). Alternating pairs: per setting one request that captures
its graph if it has to, then the timed request that replays.

    python tools/time_negative_regions.py [--config sd15|tiny] [--steps 30] [--pairs 3] [--only on|off]

--only: time one setting alone (a kernel trace of it: rocprofv3 --kernel-trace --stats -- python tools/time_negative_regions.py --only on).
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from PIL import Image  # noqa: E402

import pww_hip  # noqa: E402
import paint_with_words as pw  # noqa: E402
import pww_cases as cases  # noqa: E402

NEG_PROMPT = "blurry photo of a tree next to a dog, low quality"
NEG_CONTEXT = {(13, 255, 0): "tree,1.5", (255, 255, 255): "dog,1.0"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--only", choices=["on", "off"], default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    pww_hip.enable_miopen_find()
    tools = cases.build_tools(a.config, dtype=torch.bfloat16, device=dev, scheduler="plms")
    tools[1].to(memory_format=torch.channels_last)
    img = Image.fromarray(cases.load_example_rgb())
    kw = dict(color_map_image=img, input_prompt=cases.RUNNER_PROMPT, num_inference_steps=a.steps, guidance_scale=7.5, seed=0, device=dev,
              weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True, unconditional_input_prompt=NEG_PROMPT)

    def run(negative):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), negative_color_context=dict(NEG_CONTEXT) if negative else None,
                            negative_strength=a.strength, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if a.only is not None:
        run(a.only == "on")        # warm-up: MIOpen find, graph capture
        ts = [run(a.only == "on") for _ in range(a.pairs)]
        print("negative context %s: %s images/s" % (a.only, ", ".join("%.3f" % (1 / t) for t in ts)))
        return
    run(False)                     # warm-up: MIOpen find
    run(True)
    ratios = []
    for i in range(a.pairs):
        run(False)
        t_off = run(False)
        run(True)
        t_on = run(True)
        ratios.append(t_on / t_off)
        print("pair %d: no negative context %.3f images/s (%.1f ms), 2-region negative context %.3f images/s (%.1f ms), with / without time = %.3f"
              % (i, 1 / t_off, t_off * 1e3, 1 / t_on, t_on * 1e3, t_on / t_off), flush=True)
    print("time ratio with / without a negative context over %d pairs: %s" % (a.pairs, ", ".join("%.3f" % r for r in ratios)))


if __name__ == "__main__":
    main()
