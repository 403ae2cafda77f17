#!/usr/bin/env python
"""What LoRA adapters cost (profiles/lora.md).

1. The low-rank kernel alone (pww_lora_fwd, libpww_hip_lora.so) on the update shapes of the SD1.5 UNet at a K = 2 request's 4 rows, at
   ranks 8 and 64 (padded 32 / 64), every row with an adapter, against the stock-torch formula (ops.lora_update_torch) on the same
   operands. Both are captured into a hipGraph of ITERS launches and replayed: time per launch without host overhead. The table also states
   the launch's grid (workgroups) as the library plans it.
2. BASELINE config 2's shape -- SD1.5 UNet topology, 512 x 512, bf16, 30 PLMS steps, CFG 7.5, batch 1, hipGraph mode, channels_last,
   MIOpen find mode -- as images/s in alternating rounds: no adapter loaded; one global adapter; K = 2 region prompts with an adapter each
   (against K = 2 region prompts without adapters).

    python tools/time_region_loras.py [--config sd15|tiny] [--steps 30] [--rounds 3] [--kernel-only] [--out profiles/lora.md]
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
import lora_cases as L  # noqa: E402
from pww_hip import ops, lora  # noqa: E402

ITERS = 50
# (what, T tokens, K in-features, N out-features, segments) of the SD1.5 UNet's attention projections, per resolution level
SHAPES = [("attn1 q+k+v", T, C, 3 * C, 3) for T, C in ((4096, 320), (1024, 640), (256, 1280), (64, 1280))] + \
         [("attn2 k+v", 77, 768, 2 * C, 2) for C in (320, 640, 1280)] + \
         [("to_q / to_out", T, C, C, 1) for T, C in ((4096, 320), (1024, 640), (256, 1280), (64, 1280))]
REGIONS = dict(L.REGIONS2)


def plan_workgroups(R, T, N, n_seg):
    """The grid pww_lora_fwd launches (csrc/pww_lora.hip, lora_plan): 64-token tiles x segments x column chunks x rows."""
    seg, tt = N // n_seg, -(-T // 64)
    cw = -(-seg // 32) * 32
    while R * tt * n_seg * -(-seg // cw) < 256 and cw > 64:
        cw = -(-(cw // 2) // 32) * 32
    return R * tt * n_seg * -(-seg // cw), cw


def replay_us(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        g.replay()
        stop.record()
        torch.cuda.synchronize()
        best = min(best, start.elapsed_time(stop) * 1e3 / ITERS)
    return best


def time_kernel(dev, dtype, R=4):
    lines = ["| update | T | K | N / segments | padded rank | workgroups (chunk) | kernel us | torch formula us | kernel / torch |", "|---|---|---|---|---|---|---|---|---|"]
    for what, T, K, N, n_seg in SHAPES:
        for rank in (32, 64):
            g = torch.Generator().manual_seed(T + K + N + rank)
            x = torch.randn(R, T, K, generator=g).to(dev, dtype)
            y = torch.randn(R, T, N, generator=g).to(dev, dtype)
            A = (torch.randn(2, n_seg, rank, K, generator=g) / K ** 0.5).to(dev, dtype)
            B = (torch.randn(2, n_seg, N // n_seg, rank, generator=g) / rank ** 0.5).to(dev, dtype)
            rows = L.Rows([0, 1, 0, 1], [1.0, 0.5, -0.5, 1.0], dev)
            assert ops.lora_takes(y, x, A, B, n_seg)
            tk = replay_us(lambda: ops.lora_update(y, x, (A, B), rows, n_seg))
            tt = replay_us(lambda: ops.lora_update_torch(y, x, A, B, rows.row_adapter, rows.row_scale, n_seg))
            wg, cw = plan_workgroups(R, T, N, n_seg)
            lines.append("| %s | %d | %d | %d / %d | %d | %d (%d) | %.1f | %.1f | %.2f |" % (what, T, K, N, n_seg, rank, wg, cw, tk, tt, tk / tt))
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    out = ["## The kernel alone: us per launch, bf16, 4 rows, hipGraph replay of %d launches" % ITERS, ""] + time_kernel(dev, torch.bfloat16)
    if not a.kernel_only:
        pww_hip.enable_miopen_find()
        tools = cases.build_tools(a.config, dtype=torch.bfloat16, device=dev, scheduler="plms")
        tools[1].to(memory_format=torch.channels_last)
        img = Image.fromarray(cases.load_example_rgb())
        kw = dict(color_map_image=img, input_prompt=cases.RUNNER_PROMPT, num_inference_steps=a.steps, guidance_scale=7.5, seed=0, device=dev,
                  weight_function=cases.weight_fn_runner, preloaded_utils=tools, return_latents=True)
        a_f = L.kohya_dict(L.make_factors(tools[1], seed=11, rank=8, gain=0.5))
        b_f = L.kohya_dict(L.make_factors(tools[1], seed=12, rank=8, gain=0.5))
        colors = list(REGIONS)
        settings = {"no adapter loaded": (False, {}),
                    "one global adapter": (True, dict(lora="a")),
                    "K = 2 regions, no adapter loaded": (False, dict(region_prompts=REGIONS)),
                    "K = 2 regions, an adapter each": (True, dict(region_prompts=REGIONS, region_loras={colors[0]: "a", colors[1]: "b"}))}

        def run(name):
            loaded, more = settings[name]
            have = bool(lora.loras(tools[1]))
            if loaded and not have:
                lora.load_lora(tools[1], a_f, "a"), lora.load_lora(tools[1], b_f, "b")
            if not loaded and have:
                lora.unload_lora(tools[1], "a"), lora.unload_lora(tools[1], "b")
            pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), **more, **kw)       # captures its graph if it has to
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), **more, **kw)       # replays
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        for name in settings:
            run(name)                      # warm-up: MIOpen find at this batch size
        times = {name: [] for name in settings}
        for i in range(a.rounds):
            for name in settings:
                times[name].append(run(name))
            print("round %d: %s" % (i, ", ".join("%s %.1f ms" % (n, t[-1] * 1e3) for n, t in times.items())), flush=True)
        out += ["", "## Config-2-like request (%s, %d steps, bf16, hipGraph mode), alternating rounds" % (a.config, a.steps), "",
                "| setting | ms per image (sorted) | images/s (median) |", "|---|---|---|"]
        for name, ts in times.items():
            ms = sorted(t * 1e3 for t in ts)
            out.append("| %s | %s | %.3f |" % (name, ", ".join("%.1f" % t for t in ms), 1e3 / ms[len(ms) // 2]))
        out.append("")
        out.append("lora.stats() over the run: %s" % lora.stats())
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
