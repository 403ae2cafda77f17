#!/usr/bin/env python
"""What a long prompt costs end to end (profiles/long_prompts.md): BASELINE config 2's shape -- SD1.5 UNet topology, 512 x 512, bf16, the
5-region example map, 30 PLMS steps, CFG 7.5, batch 1, hipGraph mode, channels_last, MIOpen find mode -- with the 77-token prompt of the
example and with the same request spread over 225 tokens (three chunks, 231 keys; the five region phrases sit in chunks 1, 2 and 3).
Alternating pairs: per setting one request that captures its graph if it has to, then the timed request that replays.

    python tools/time_long_request.py [--config sd15|tiny] [--steps 30] [--pairs 3]
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


def long_prompt():
    """225 content tokens: the example's words, 'tree' at position ~100, 'sky' and 'ground' past 150, filler between them."""
    fill = lambda a, b: " ".join("detail%d" % i for i in range(a, b))      # noqa: E731
    return ("realistic photo of a dog, cat, " + fill(0, 92) + " tree, " + fill(92, 140) + " with beautiful sky, " + fill(140, 200)
            + " on sandy ground " + fill(200, 206))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    pww_hip.enable_miopen_find()
    tools = cases.build_tools(a.config, dtype=torch.bfloat16, device=dev, scheduler="plms")
    tools[1].to(memory_format=torch.channels_last)
    img = Image.fromarray(cases.load_example_rgb())
    kw = dict(color_map_image=img, num_inference_steps=a.steps, guidance_scale=7.5, seed=0, device=dev, weight_function=cases.weight_fn_runner,
              preloaded_utils=tools, return_latents=True)
    lp = long_prompt()
    from pww_hip import conditioning
    print("long prompt: %d content tokens, %d chunks" % (len(conditioning._content_ids(tools[3], lp)), conditioning.prompt_chunk_count(tools[3], lp, 3)))

    def run(long):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), input_prompt=lp if long else cases.RUNNER_PROMPT,
                            max_prompt_chunks=3 if long else 1, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(False)                     # warm-up: MIOpen find
    run(True)
    ratios = []
    for i in range(a.pairs):
        run(False)
        t77 = run(False)
        run(True)
        t231 = run(True)
        ratios.append(t231 / t77)
        print("pair %d: 77 tokens %.3f images/s (%.1f ms), 231 tokens %.3f images/s (%.1f ms), 231 / 77 time = %.3f" % (i, 1 / t77, t77 * 1e3, 1 / t231, t231 * 1e3, t231 / t77), flush=True)
    print("time ratio 231 / 77 tokens over %d pairs: %s" % (a.pairs, ", ".join("%.3f" % r for r in ratios)))


if __name__ == "__main__":
    main()
