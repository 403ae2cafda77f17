"""Attention-map demo (GPU): the README's five-region example (tests/golden/example_input.png, the runner's prompt and weight function,
stand-in weights) with pww_hip.record_attention_maps(), written as ONE PNG sheet -- the colour map beside one heat map per region
phrase -- plus images/s with the recorder off and on (alternating pairs, hipGraph mode, replayed requests).

    python tools/attn_maps_demo.py [--config sd15|tiny] [--steps 30] [--pairs 3] [--out attn_maps_demo.png]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default="attn_maps_demo.png")
    a = ap.parse_args()
    dev = "cuda:0"
    pww_hip.enable_miopen_find()
    tools = cases.build_tools(a.config, dtype=torch.bfloat16, device=dev, scheduler="plms")
    tools[1].to(memory_format=torch.channels_last)
    img = Image.fromarray(cases.load_example_rgb())
    kw = dict(color_map_image=img, input_prompt=cases.RUNNER_PROMPT, num_inference_steps=a.steps, guidance_scale=7.5, seed=0, device=dev,
              weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True)

    def run(record):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if record:
            with pww_hip.record_attention_maps() as rec:
                pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), **kw)
        else:
            rec = None
            pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rec

    run(False)                     # warm-up: MIOpen find
    rec = None
    for i in range(a.pairs):
        # toggling the recorder re-captures the graph (it is part of the graph's geometry): per setting one request that captures, then the
        # timed one that replays
        run(False)
        t_off, _ = run(False)
        run(True)
        t_on, rec = run(True)
        print("pair %d: recorder off %.3f images/s, on %.3f images/s, on / off = %.3f" % (i, 1 / t_off, 1 / t_on, t_off / t_on), flush=True)

    maps = rec.maps()
    print("resolutions", maps.resolutions, "counts", maps.counts)
    phrases = [v.split(",")[0] for v in cases.RUNNER_CONTEXT.values()]
    tile = 192
    sheet = Image.new("RGB", (tile * (1 + len(phrases)), tile), "black")
    sheet.paste(img.resize((tile, tile), Image.NEAREST), (0, 0))
    for i, ph in enumerate(phrases):
        sheet.paste(maps.to_pil(ph)[0].resize((tile, tile), Image.BILINEAR).convert("RGB"), (tile * (1 + i), 0))
    sheet.save(a.out)
    print("wrote %s: colour map | %s" % (a.out, " | ".join(phrases)))


if __name__ == "__main__":
    main()
