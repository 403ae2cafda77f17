#!/usr/bin/env python
"""What a per-head / per-row weight function costs per cross-attention call on the two routes (profiles/scoped_stats.md):

    wf_head = 0.4 * w * log(1 + sigma) * qk.amax(dim=(1, 2), keepdim=True)
    wf_row  = 0.5 * w * log(1 + sigma^2) * qk.std(dim=-1, keepdim=True)

on the launches of libpww_hip_scope.so (PWW_SCOPED_STATS=1, the default) and on the materialised route (PWW_SCOPED_STATS=0: Q K^T as a
tensor, the reduction and the products as torch ops, a dense [B * heads, N, M] fp32 bias into the general kernel). One call =
pww_hip.attention.pww_attention on a CrossAttention stand-in of the layer's shape with a dict context (to_q, the cached K|V projection,
the weight function, the attention launches): the part of the two routes that differs plus the projection they share. The prompt is
repeated per image: the materialised route needs a key row per image.

Timing: device event pairs around `--calls` back-to-back calls, the two routes alternating, `--rounds` rounds after a warm-up round; the
figure is the median over the rounds of (elapsed / calls). It includes the gaps between the launches of a call (the materialised route is
seven launches, the new one two or three), which is what a step of the sampler pays in eager and folded mode.

Kernel-only times: the same `--calls` calls captured into ONE hipGraph per route and replayed -- the kernels of a call back to back,
no host between them -- timed by an event pair around the replay; the to_q GEMM both routes share is captured alone the same way and
printed beside them, so that (route - to_q) is what the weight function and the attention launches cost on the device.

Shapes: the headline workload's finest level at batch 1 (1 x 8 heads x 4096 x 77, d = 40, bf16), 16 folded rows of the same, and the
N = 64, d = 160 layer. Then, in hipGraph mode on the tiny tools: captures and images/s of a 30-step request on either route.

    python tools/time_scoped_stats.py [--calls 20] [--rounds 7] [--steps 30] [--skip-loop]
"""
import argparse
import math
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from PIL import Image  # noqa: E402

import paint_with_words as pw  # noqa: E402
import pww_cases as cases  # noqa: E402
from pww_hip import attention as A  # noqa: E402


def wf_head(w, s, qk):
    return 0.4 * w * math.log(1 + s) * qk.amax(dim=(1, 2), keepdim=True)


def wf_row(w, s, qk):
    return 0.5 * w * math.log(1 + s ** 2) * qk.std(dim=-1, keepdim=True)


SHAPES = [("batch 1, N 4096, d 40", 1, 4096, 320, 8), ("16 rows, N 4096, d 40", 16, 4096, 320, 8), ("batch 1, N 64, d 160", 1, 64, 1280, 8)]


def time_calls(a):
    from sd_standin import CrossAttention
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    print("| shape | function | scoped route, us / call | materialised route, us / call | materialised / scoped |")
    print("|---|---|---|---|---|")
    for name, B, N, C, H in SHAPES:
        torch.manual_seed(0)
        attn = CrossAttention(C, 768, H, C // H).to(dev, dtype).requires_grad_(False)
        attn.to_q.weight.mul_(3.0)
        hidden = torch.randn(B, N, C, device=dev, dtype=dtype)
        w = ((torch.rand(N, 77, device=dev) < 0.15).float() * torch.rand(N, 77, device=dev) * 1.5)
        w[:, 20:] = 0.0
        for fname, wf in (("head", wf_head), ("row", wf_row)):
            ctx = {"CONTEXT_TENSOR": torch.randn(1, 77, 768, device=dev, dtype=dtype).expand(B, -1, -1).contiguous(), "CROSS_ATTENTION_WEIGHT_%d" % N: w, "SIGMA": 7.84,
                   "WEIGHT_FUNCTION": wf, A.KV_CACHE: {}}
            times = {True: [], False: []}
            for rnd in range(a.rounds + 1):
                for scoped in (True, False):
                    A.SCOPED_STATS = scoped
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        out = A.pww_attention(attn, hidden, ctx)
                    e1.record()
                    e1.synchronize()
                    if rnd:
                        times[scoped].append(e0.elapsed_time(e1) * 1e3 / a.calls)
            A.SCOPED_STATS = True
            new, old = statistics.median(times[True]), statistics.median(times[False])
            print("| %s | %s | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2f |" % (name, fname, new, min(times[True]), max(times[True]), old,
                                                                                min(times[False]), max(times[False]), old / new), flush=True)
            del out


def _graph_us(fn, calls, rounds):
    """us per call of `fn` from a replayed hipGraph that holds `calls` of them (median, min, max over `rounds` replays after a warm-up)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            keep = fn()
    ts = []
    for rnd in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        if rnd:
            ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    del keep
    return statistics.median(ts), min(ts), max(ts)


def time_kernels(a):
    from sd_standin import CrossAttention
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    print()
    print("| shape | function | scoped route, us / call (graph replay) | materialised route, us / call (graph replay) | to_q alone, us | materialised / scoped |")
    print("|---|---|---|---|---|---|")
    for name, B, N, C, H in SHAPES:
        torch.manual_seed(0)
        attn = CrossAttention(C, 768, H, C // H).to(dev, dtype).requires_grad_(False)
        attn.to_q.weight.mul_(3.0)
        hidden = torch.randn(B, N, C, device=dev, dtype=dtype)
        w = ((torch.rand(N, 77, device=dev) < 0.15).float() * torch.rand(N, 77, device=dev) * 1.5)
        w[:, 20:] = 0.0
        toq = _graph_us(lambda: attn.to_q(hidden), a.calls, a.rounds)
        for fname, wf in (("head", wf_head), ("row", wf_row)):
            ctx = {"CONTEXT_TENSOR": torch.randn(1, 77, 768, device=dev, dtype=dtype).expand(B, -1, -1).contiguous(), "CROSS_ATTENTION_WEIGHT_%d" % N: w, "SIGMA": 7.84,
                   "WEIGHT_FUNCTION": wf, A.KV_CACHE: {}}
            res = {}
            for scoped in (True, False):
                A.SCOPED_STATS = scoped
                A.pww_attention(attn, hidden, ctx)      # (eager once: the K|V cache and the library are there before the capture)
                res[scoped] = _graph_us(lambda: A.pww_attention(attn, hidden, ctx), a.calls, a.rounds)
            A.SCOPED_STATS = True
            print("| %s | %s | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.1f | %.2f |" % ((name, fname) + res[True] + res[False] + (toq[0], res[False][0] / res[True][0])),
                  flush=True)


def time_loop(a):
    dev = "cuda:0"
    img = Image.fromarray(cases.load_example_rgb())
    import importlib
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    pww_mod.DEFAULT_MODE = "graph"
    print()
    print("| function | route | captures | images/s (30-step request after the capturing one) |")
    print("|---|---|---|---|")
    for fname, wf in (("head", wf_head), ("row", wf_row)):
        for scoped in (True, False):
            A.SCOPED_STATS = scoped
            tools = cases.build_tools("tiny", dtype=torch.bfloat16, device=dev)
            kw = dict(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=img, input_prompt=cases.RUNNER_PROMPT, num_inference_steps=a.steps,
                      guidance_scale=7.5, seed=0, device=dev, weight_function=wf, preloaded_utils=tools, return_latents=True)
            pw.paint_with_words(**kw)
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pw.paint_with_words(**kw)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            captures = tools[1]._pww_samplers[(id(tools[4]), "graph")]._graphed.captures
            print("| %s | %s | %d | %s |" % (fname, "scoped" if scoped else "materialised", captures, ", ".join("%.2f" % (1 / t) for t in ts)), flush=True)
    A.SCOPED_STATS = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    warnings.filterwarnings("ignore", message=".*materialising.*")
    time_calls(a)
    time_kernels(a)
    if not a.skip_loop:
        time_loop(a)


if __name__ == "__main__":
    main()
