#!/usr/bin/env python
"""Per-shape timing of conv2 + conv_shortcut of the SD1.5 UNet's fourteen channel-changing ResnetBlock2D at 2 rows: the unfused sequence
(the 1 x 1 shortcut as a stock GEMM with its bias, then ops.conv3x3 with bias and residual) against ops.conv3x3_shortcut
(csrc/pww_conv_tail.hip) at the library's tile / split choice and, with --sweep, at the alternatives. Every call is captured once and
replayed 20x back to back from a hipGraph, best of 5 (event interval / 20: includes the dispatch gaps, no host in the loop). Also checks
each fused result against an fp64 evaluation of the same rounded inputs (max |err| / max |ref|).

Usage: python tools/time_convtail.py [--sweep] [--dtype bf16] [out.md]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

# (C2 = the block's input channels, Cout = conv2's channels, size, count per forward) at 512 x 512 (latent 64 x 64)
SHAPES = [(2560, 1280, 8, 3), (2560, 1280, 16, 2), (1920, 1280, 16, 1), (640, 1280, 16, 1),
          (1920, 640, 32, 1), (1280, 640, 32, 1), (960, 640, 32, 1), (320, 640, 32, 1), (960, 320, 64, 1), (640, 320, 64, 2)]
SPLITS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24)


def replay_us(call, reps=20):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            call()
    g.replay()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    del g
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--sweep", action="store_true", help="also time tile_n 64 / 128 / 160 and a range of K splits")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    import pww_hip
    from pww_hip import ops
    pww_hip.load_library()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    cl = torch.channels_last
    rows = args.rows
    lines = ["| rows | C2 -> Cout | size | n/fwd | shortcut GEMM us | conv2 + residual us | unfused us | fused us | fused / unfused | tile_n, split | err | best sweep | sweep |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    tot = [0.0, 0.0, 0.0]
    torch.manual_seed(0)
    for C2, Cout, S, count in SHAPES:
        h = torch.randn(rows, Cout, S, S, device=dev).to(dt).contiguous(memory_format=cl)
        x = torch.randn(rows, C2, S, S, device=dev).to(dt).contiguous(memory_format=cl)
        w = (torch.randn(Cout, Cout, 3, 3, device=dev) / (3 * Cout ** 0.5)).to(dt).contiguous(memory_format=cl)
        w2 = (torch.randn(Cout, C2, 1, 1, device=dev) / C2 ** 0.5).to(dt)
        b, b2 = (torch.randn(Cout, device=dev) * 0.1).to(dt), (torch.randn(Cout, device=dev) * 0.1).to(dt)

        def shortcut():
            y = F.linear(x.permute(0, 2, 3, 1).reshape(rows * S * S, C2), w2.reshape(Cout, C2), b2)
            return y.view(rows, S, S, Cout).permute(0, 3, 1, 2)
        r = shortcut()
        t_sc = replay_us(shortcut)
        t_conv = replay_us(lambda: ops.conv3x3(h, w, b, residual=r))
        t_unfused = replay_us(lambda: ops.conv3x3(h, w, b, residual=shortcut()))
        fused = lambda tn=0, sk=0: ops.conv3x3_shortcut(h, w, b, x, w2, b2, tile_n=tn, splitk=sk)  # noqa: E731
        y = fused().double()
        ref = (F.conv2d(h.double(), w.double(), None, 1, 1) + F.conv2d(x.double(), w2.double()) + (b.double() + b2.double())[None, :, None, None])
        err = ((y - ref).abs().max() / ref.abs().max()).item()
        t_fused = replay_us(fused)
        d = ops._lib.ConvTailDesc(ops.ctypes.sizeof(ops._lib.ConvTailDesc), ops._DT[dt], rows, S, S, Cout, C2, Cout, 0, 0)
        nbytes = ops._lib.load_convtail().pww_convtail_workspace_bytes(ops.ctypes.byref(d))
        split = nbytes // (4 * rows * S * S * Cout) if nbytes else 1
        best = cells = ""
        if args.sweep:
            res = []
            nslab = (9 * Cout + C2) // 64
            for tn in (64, 128, 160):
                if Cout % tn:
                    continue
                for sk in SPLITS:
                    if sk > nslab // 4 or rows * S * S * Cout * sk * 4 > 1 << 28:
                        continue
                    res.append((replay_us(lambda: fused(tn, sk)), tn, sk))
            cells = " ".join("%d/%d:%.1f" % (tn, sk, t) for t, tn, sk in res)
            res.sort()
            best = "%.1f us @ %d, %d" % res[0] if res else ""
        tot[0] += count * t_sc
        tot[1] += count * t_unfused
        tot[2] += count * t_fused
        lines.append("| %d | %d->%d | %d | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %s, %d | %.1e | %s | %s |" % (
            rows, C2, Cout, S, count, t_sc, t_conv, t_unfused, t_fused, t_fused / t_unfused, "auto", split, err, best, cells))
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("rows %d: per UNet forward (count-weighted) shortcut GEMMs %.0f us, unfused %.0f us, fused %.0f us (%.0f us less)"
                 % (rows, tot[0], tot[1], tot[2], tot[1] - tot[2]))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
