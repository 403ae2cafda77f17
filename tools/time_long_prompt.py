#!/usr/bin/env python
"""Cross-attention launches of a long prompt (154 / 231 keys), per SD1.5 layer class at 2 and 16 folded rows (profiles/long_prompts.md):

  three-launch   the route such a call took before libpww_hip_long.so: pww_qk_reduce (ticket + reduction kernels), then the general kernel
                 reading the fp32 map from HBM score by score (ops.qk_stats + ops.attention(stat=(stats, kind, scalar)))
  long pair      pww_long_qk_parts + pww_long_cross_attn_fwd_parts
  77 tokens      pww_qk_parts + pww_cross_attn_fwd_parts of the same layer, for orientation

pww_qk_reduce's kernels carry no dispatch stamps, so all three columns are measured alike: the route's launches, REPS times, captured into one
hipGraph; wall time of a replay / REPS, median of 7 replays (device events; no host launch cost, the gaps between dependent kernels included).
The kernel-only stamps of the new pair (pww_long_profile_arm) are printed beside it.

    python tools/time_long_prompt.py [--out FILE.md]
"""
import argparse
import ctypes
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from pww_hip import _lib, ops      # noqa: E402

REPS = 20
LAYERS = [(4096, 8, 40), (1024, 8, 80), (256, 8, 160), (64, 8, 160)]      # (N, heads, head dim) of SD1.5's four levels


def graph_us(fn):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(REPS):
                fn()
    times = []
    for _ in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / REPS)
    return statistics.median(times[1:])


def stamp_us(fn):
    lib = _lib.load_long()
    out = []
    for _ in range(8):
        _lib.check(lib.pww_long_profile_arm(), "pww_long_profile_arm", lib)
        fn()
        us = ctypes.c_float()
        _lib.check(lib.pww_long_profile_elapsed_us(ctypes.byref(us)), "pww_long_profile_elapsed_us", lib)
        out.append(us.value)
    return statistics.median(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f16"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(5)
    kind, scalar = ops.STAT_MAX, 0.4 * math.log(1 + 7.84)
    lines = ["| N | heads x d | rows | M | three-launch us | long pair us | ratio | long pair, kernel stamps (parts + attention) us | 77 tokens us |",
             "|---|---|---|---|---|---|---|---|---|"]
    worst = 0.0
    for (N, H, D) in LAYERS:
        for B in (2, 16):
            q = torch.randn(B, N, H * D, generator=g).to(dev, dtype)
            gate = torch.cat([torch.ones(B // 2), torch.zeros(B // 2)]).to(dev)
            res = {}
            for M in (154, 231, 77):
                k = torch.randn(1, M, H * D, generator=g).to(dev, dtype)
                v = torch.randn(1, M, H * D, generator=g).to(dev, dtype)
                w = torch.zeros(N, M)
                cols = [c for c in (3, 40, 100, 170, 220) if c < M]
                for c in cols:
                    w[torch.rand(N, generator=g) < 0.3, c] = 1.0
                w = w.to(dev)
                bias_cols = (max(cols) + 16) // 16 * 16
                scale = D ** -0.5
                if M == 77:
                    def short():
                        parts = ops.qk_parts(q, k, H, kind, gate=gate, gated=B // 2)
                        return ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate, stat=(None, kind, scalar), parts=parts, bias_cols=bias_cols, gated=B // 2)
                    res[M] = graph_us(short)
                    continue

                def old():
                    st = ops.qk_stats(q, k, H)
                    return ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate, stat=(st, kind, scalar))

                def new():
                    parts = ops.long_qk_parts(q, k, H, kind, gate=gate, gated=B // 2)
                    return ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate, stat=(None, kind, scalar), parts=parts, bias_cols=bias_cols, gated=B // 2)
                parts = ops.long_qk_parts(q, k, H, kind, gate=gate, gated=B // 2)
                s_parts = stamp_us(lambda: ops.long_qk_parts(q, k, H, kind, gate=gate, gated=B // 2))
                s_attn = stamp_us(lambda: ops.attention(q, k, v, H, scale, bias=w, bias_coeff=gate, stat=(None, kind, scalar), parts=parts, bias_cols=bias_cols, gated=B // 2))
                res[M] = (graph_us(old), graph_us(new), s_parts, s_attn)
            for M in (154, 231):
                t_old, t_new, s_parts, s_attn = res[M]
                worst = max(worst, t_new / t_old)
                lines.append("| %d | %d x %d | %d | %d | %.1f | %.1f | %.2f | %.1f + %.1f | %.1f |" % (N, H, D, B, M, t_old, t_new, t_new / t_old, s_parts, s_attn, res[77]))
                print(lines[-1], flush=True)
    lines.append("")
    lines.append("largest long pair / three-launch ratio: %.2f (%s)" % (worst, args.dtype))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if worst <= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
