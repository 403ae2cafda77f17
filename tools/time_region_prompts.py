#!/usr/bin/env python
"""What region prompts cost (profiles/region_prompts.md): BASELINE config 2's shape -- SD1.5 UNet topology, 512 x 512, bf16, the 5-region
example map, 30 PLMS steps, CFG 7.5, batch 1, hipGraph mode, channels_last, MIOpen find mode -- with K = 0, 2 and 5 region prompts (K more
rows of every UNet evaluation), in alternating rounds: per setting one request that captures its graph if it has to, then the timed request
that replays. Then the blend launch alone (pww_regions_combine) against the torch composition of the same formula.

    python tools/time_region_prompts.py [--config sd15|tiny] [--steps 30] [--rounds 3] [--only K] [--combine-only]

--only K: time one setting alone (a kernel trace of it: rocprofv3 --kernel-trace --stats -- python tools/time_region_prompts.py --only 5).
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
from pww_hip import ops  # noqa: E402
from pww_hip.sampler import region_blend_fp32  # noqa: E402

REGIONS = {(13, 255, 0): "an old oak tree with autumn leaves", (255, 255, 255): "a white fluffy dog, studio photo",
           (90, 206, 255): "stormy sky with dark clouds", (0, 0, 0): "a black cat sleeping", (74, 18, 1): "wet cobblestone street at night"}


def time_combine(dev, dtype, iters=200):
    """us per call of ops.region_combine and of the torch composition of the same formula, K = 2 and 5, one 64 x 64 x 4 latent."""
    for K in (2, 5):
        g = torch.Generator().manual_seed(K)
        eps = torch.randn(K + 2, 4, 64, 64, generator=g).to(dev, dtype)
        masks = (torch.rand(1, K, 64, 64, generator=g) / K).to(dev)
        weights, scales = torch.rand(1, K, generator=g).to(dev), (1 + 10 * torch.rand(1, K, generator=g)).to(dev)
        out = {}
        for name, f in (("pww_regions_combine", ops.region_combine), ("torch composition", region_blend_fp32)):
            for _ in range(10):
                f(eps, masks, weights, scales, 7.5)
            torch.cuda.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                f(eps, masks, weights, scales, 7.5)
            stop.record()
            torch.cuda.synchronize()
            out[name] = start.elapsed_time(stop) * 1e3 / iters
        same = torch.equal(ops.region_combine(eps, masks, weights, scales, 7.5), region_blend_fp32(eps, masks, weights, scales, 7.5))
        print("blend of one step, K = %d, %s, [%d, 4, 64, 64]: %s (stream time per call, launch overhead included); bit-identical: %s"
              % (K, str(dtype)[6:], K + 2, ", ".join("%s %.1f us" % kv for kv in out.items()), same), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, choices=[0, 2, 5], default=None)
    ap.add_argument("--combine-only", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    if a.combine_only:
        time_combine(dev, torch.bfloat16)
        return
    pww_hip.enable_miopen_find()
    tools = cases.build_tools(a.config, dtype=torch.bfloat16, device=dev, scheduler="plms")
    tools[1].to(memory_format=torch.channels_last)
    img = Image.fromarray(cases.load_example_rgb())
    kw = dict(color_map_image=img, input_prompt=cases.RUNNER_PROMPT, num_inference_steps=a.steps, guidance_scale=7.5, seed=0, device=dev,
              weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True)

    def run(K):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), region_prompts=dict(list(REGIONS.items())[:K]) if K else None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    settings = (0, 2, 5) if a.only is None else (a.only,)
    for K in settings:
        run(K)                     # warm-up: MIOpen find at this batch size, graph capture
    times = {K: [] for K in settings}
    for i in range(a.rounds):
        for K in settings:
            if len(settings) > 1:
                run(K)             # captures again (the row count is part of the graph's signature)
            times[K].append(run(K))
        print("round %d: %s" % (i, ", ".join("K = %d: %.1f ms per image" % (K, times[K][-1] * 1e3) for K in settings)), flush=True)
    for K in settings:
        ms = sorted(t * 1e3 for t in times[K])
        line = "K = %d (%d rows per UNet call): ms per image %s" % (K, K + 2, ", ".join("%.1f" % t for t in ms))
        if K and 0 in times:
            line += "; median / median of K = 0: %.2f" % (ms[len(ms) // 2] / sorted(times[0])[len(times[0]) // 2] / 1e3)
        print(line)
    time_combine(dev, torch.bfloat16)


if __name__ == "__main__":
    main()
