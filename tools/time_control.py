#!/usr/bin/env python
"""What a ControlNet costs, and what the grouped launch buys (profiles/control.md).

(a) The grouped launch alone (pww_control_fwd, libpww_hip_control.so): the thirteen zero convolutions of the SD1.5 topology at 2 rows, bf16,
    with the scale and the add into the skips -- against the stock sequence it replaces (13 x the 1 x 1 convolution as a GEMM over the
    [B H W, C] view, 13 x the multiplication by the scale word, 13 x the add) and against 13 ops.linear launches with the residual in the
    epilogue (no scale: the per-problem native launch). Each variant is captured into a hipGraph of ITERS repetitions; the graphs are
    replayed in alternating rounds, and the table gives the median with the spread (min .. max) over the rounds.
(b) A whole request -- SD1.5 UNet + ControlNet topology, 512 x 512, bf16, hipGraph mode, channels_last -- with the ControlNet on the native
    route, with PWW_CONTROL=0, and without a ControlNet, in alternating rounds; and the native route with the guidance window closed after
    half of the steps (hipGraph mode keeps running the ControlNet with the scale word at 0: the cost of the idle ControlNet).

    python tools/time_control.py [--config sd15|request] [--steps 30] [--rounds 5] [--kernel-only] [--out profiles/control.md]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from PIL import Image  # noqa: E402

import pww_hip  # noqa: E402
import paint_with_words as pw  # noqa: E402
import pww_cases as cases  # noqa: E402
import control_cases as CC  # noqa: E402
from pww_hip import ops, controlnet  # noqa: E402

ITERS = 20
# (channels, latent side) of the thirteen hidden states of the SD1.5 ControlNet at a 64 x 64 latent
SD15 = [(320, 64)] * 3 + [(320, 32)] + [(640, 32)] * 2 + [(640, 16)] + [(1280, 16)] * 2 + [(1280, 8)] * 4


def spread(values):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(values), min(values), max(values))


def graph_of(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    g.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / ITERS


def time_launch(dev, dtype, rows, rounds):
    gen = torch.Generator().manual_seed(5)
    hs, skips, convs = [], [], []
    for C, side in SD15:
        hs.append(torch.randn(rows, C, side, side, generator=gen).to(dev, dtype).contiguous(memory_format=torch.channels_last))
        skips.append(torch.randn(rows, C, side, side, generator=gen).to(dev, dtype).contiguous(memory_format=torch.channels_last))
        convs.append(nn.Conv2d(C, C, 1).to(device=dev, dtype=dtype).requires_grad_(False))
    word = torch.tensor([0.8], dtype=torch.float32, device=dev)
    assert ops.control_takes(hs, convs, word, skips)
    outs = ops.control_residuals(hs, convs, word, skips=skips)
    views = [(h.permute(0, 2, 3, 1), s.permute(0, 2, 3, 1), c.weight.reshape(c.out_channels, c.in_channels), c.bias) for h, s, c in zip(hs, skips, convs)]
    out_views = [o.permute(0, 2, 3, 1) for o in outs]

    def grouped():
        ops.control_residuals(hs, convs, word, skips=skips, outs=outs)

    def stock():
        s = word.to(dtype)
        return [sk + F.linear(h, w, b) * s for h, sk, w, b in views]

    def linears():
        for (h, sk, w, b), o in zip(views, out_views):
            ops.linear(h, w, b, residual=sk, out=o)

    variants = {"grouped launch (1 launch)": grouped, "stock sequence (13 GEMM + 13 scale + 13 add)": stock, "13 ops.linear residual launches (no scale)": linears}
    graphs = {k: graph_of(f) for k, f in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(replay_us(g))
    base = statistics.median(times["grouped launch (1 launch)"])
    lines = ["| variant | us per evaluation: median (min .. max) over %d alternating rounds | against the grouped launch |" % rounds, "|---|---|---|"]
    for k, ts in times.items():
        lines.append("| %s | %s | %.2f x |" % (k, spread(ts), statistics.median(ts) / base))
    wins = max(times["grouped launch (1 launch)"]) < min(times["stock sequence (13 GEMM + 13 scale + 13 add)"])
    lines += ["", "The grouped launch %s the stock sequence outside the spread (its slowest round against the stock sequence's fastest)." % ("beats" if wins else "does NOT beat")]
    return lines


def time_request(a, dev, dtype):
    from sd_standin import build_unet, build_controlnet, HashTokenizer, TinyTextEncoder, TinyVAE, PLMSScheduler, SD15_CONFIG
    cfg, side = (SD15_CONFIG, 512) if a.config == "sd15" else (CC.REQUEST_CONFIG, CC.SIDE)
    pww_hip.enable_miopen_find()
    unet = build_unet(cfg, seed=1234, dtype=dtype, device=dev, qk_gain=2.0).to(memory_format=torch.channels_last)
    net = build_controlnet(cfg, seed=1239, dtype=dtype, device=dev).to(memory_format=torch.channels_last)
    text = TinyTextEncoder(cfg["cross_attention_dim"], seed=1235).to(device=dev, dtype=dtype)
    vae, tok = TinyVAE(4, seed=1236).to(device=dev, dtype=dtype), HashTokenizer()
    cmap = Image.fromarray(cases.load_example_rgb()).resize((side, side), Image.NEAREST)
    hint = CC.control_image(1, side)
    kw = dict(color_map_image=cmap, input_prompt=cases.RUNNER_PROMPT, num_inference_steps=a.steps, guidance_scale=7.5, seed=0, device=dev,
              weight_function=cases.weight_fn_runner, return_latents=True)
    # one scheduler object per setting: each finds a sampler of its own on the UNet, so every setting keeps its captured graph across the rounds
    settings = {"no ControlNet": ("1", {}),
                "ControlNet, native route (grouped launch)": ("1", dict(controlnet=net, control_image=hint)),
                "ControlNet, PWW_CONTROL=0 (stock zero convolutions)": ("0", dict(controlnet=net, control_image=hint)),
                "ControlNet, native route, window [0, 0.5]": ("1", dict(controlnet=net, control_image=hint, control_guidance_end=0.5))}
    tools = {name: (vae, unet, text, tok, PLMSScheduler()) for name in settings}

    def run(name):
        env, more = settings[name]
        os.environ["PWW_CONTROL"] = env
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), preloaded_utils=tools[name], **more, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for name in settings:
        run(name), run(name)             # warm-up: MIOpen find, the capture
    controlnet.reset_stats()
    times = {name: [] for name in settings}
    for i in range(a.rounds):
        for name in settings:
            times[name].append(run(name) * 1e3)
        print("round %d: %s" % (i, ", ".join("%s %.1f ms" % (n, t[-1]) for n, t in times.items())), flush=True)
    os.environ.pop("PWW_CONTROL", None)
    base = statistics.median(times["no ControlNet"])
    lines = ["| setting | ms per image: median (min .. max) over %d alternating rounds | against no ControlNet |" % a.rounds, "|---|---|---|"]
    for name, ts in times.items():
        lines.append("| %s | %s | %.3f x |" % (name, spread(ts), statistics.median(ts) / base))
    lines += ["", "controlnet.stats() over the rounds: %s" % controlnet.stats()]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sd15", choices=["sd15", "request"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, dtype = "cuda:0", torch.bfloat16
    out = ["## (a) The residuals of one evaluation: SD1.5 topology, 2 rows, bf16, hipGraph replay of %d repetitions" % ITERS, ""] + time_launch(dev, dtype, 2, a.rounds)
    if not a.kernel_only:
        out += ["", "## (b) A whole request (%s, %d steps, bf16, hipGraph mode, channels_last)" % (a.config, a.steps), ""] + time_request(a, dev, dtype)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
