#!/usr/bin/env python
"""Per-shape timing of the SD1.5 UNet's 3 x 3 convolutions: the stock op (F.conv2d -> MIOpen, channels_last bf16, find mode and
PYTORCH_MIOPEN_SUGGEST_NHWC=1 as bench.py sets them) against ops.conv3x3 (csrc/pww_conv.hip) at the library's tile / split choice and at
the alternatives given with --sweep. Every call is captured once and replayed 20x back to back from a hipGraph (event interval / 20:
includes the dispatch gaps, no host in the loop). The stock Upsample2D row is interpolate + conv, the HIP row the fused gather.
Also checks each HIP result against an fp32 F.conv2d of the same rounded inputs (max |err| / max |ref|), and with --kernels lists the
kernels the stock op launches (torch.profiler over one eager call).

Usage: python tools/time_conv3x3.py [--rows 2,16] [--sweep] [--kernels] [--dtype bf16] [out.md]"""
import argparse
import os
import sys

os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", "0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_TFLOPS = 2500.0          # dense bf16 / fp16 MFMA peak of the MI355X
# (Cin, Cout, output size, stride, upsample, count per forward) of the SD1.5 UNet at 512 x 512 (latent 64 x 64)
SHAPES = [(320, 320, 64, 1, 0, 7), (640, 640, 64, 1, 1, 1), (960, 320, 64, 1, 0, 1), (640, 320, 64, 1, 0, 2),
          (320, 320, 32, 2, 0, 1), (320, 640, 32, 1, 0, 1), (640, 640, 32, 1, 0, 6), (1280, 1280, 32, 1, 1, 1), (1920, 640, 32, 1, 0, 1),
          (1280, 640, 32, 1, 0, 1), (960, 640, 32, 1, 0, 1),
          (640, 640, 16, 2, 0, 1), (640, 1280, 16, 1, 0, 1), (1280, 1280, 16, 1, 0, 6), (1280, 1280, 16, 1, 1, 1), (2560, 1280, 16, 1, 0, 2), (1920, 1280, 16, 1, 0, 1),
          (1280, 1280, 8, 2, 0, 1), (1280, 1280, 8, 1, 0, 11), (2560, 1280, 8, 1, 0, 3)]


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


def stock_kernels(call):
    from torch.profiler import profile, ProfilerActivity
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA" or getattr(e, "device_type", None) == "cuda"]
    out = []
    for n in names:
        short = n.split("(")[0][:60]
        if short not in out:
            out.append(short)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2,16")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--sweep", action="store_true", help="also time tile_n 64 / 128 / 160 and a range of K splits")
    ap.add_argument("--kernels", action="store_true", help="list the stock op's kernels per shape")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    import pww_hip
    from pww_hip import ops
    pww_hip.enable_miopen_find()
    pww_hip.load_library()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    cl = torch.channels_last
    lines = ["| rows | Cin->Cout | out | s | up | n/fwd | GFLOP | stock us | stock TF/s (%peak) | HIP us | HIP TF/s (%peak) | HIP/stock | tile_n, split | err | best sweep |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    kern_lines = []
    tot = {}
    torch.manual_seed(0)
    for rows in [int(r) for r in args.rows.split(",")]:
        for Cin, Cout, S, stride, up, count in SHAPES:
            Hin = S * stride // (2 if up else 1)
            x = torch.randn(rows, Cin, Hin, Hin, device=dev).to(dt).contiguous(memory_format=cl)
            w = (torch.randn(Cout, Cin, 3, 3, device=dev) / (3 * Cin ** 0.5)).to(dt).contiguous(memory_format=cl)
            b = (torch.randn(Cout, device=dev) * 0.1).to(dt)
            flop = 2.0 * rows * S * S * Cout * 9 * Cin
            if up:
                stock = lambda: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, 1, 1)  # noqa: E731
            else:
                stock = lambda: F.conv2d(x, w, None, stride, 1)  # noqa: E731
            t_stock = replay_us(stock)
            if args.kernels:
                kern_lines.append("| %d | %d->%d | %d | %d | %d | %s |" % (rows, Cin, Cout, S, stride, up, "<br>".join(stock_kernels(stock))))
            hip = lambda tn=0, sk=0: ops.conv3x3(x, w, b if up else None, stride=stride, upsample=bool(up), tile_n=tn, splitk=sk)  # noqa: E731
            y = hip().float()
            xr = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
            ref = F.conv2d(xr, w.float(), b.float() if up else None, stride, 1)
            err = ((y - ref).abs().max() / ref.abs().max()).item()
            t_hip = replay_us(hip)
            d = ops._lib.ConvDesc(ops.ctypes.sizeof(ops._lib.ConvDesc), ops._DT[dt], rows, Hin, Hin, Cin, Cout, stride, up, 0, 0, 0)
            nbytes = ops._lib.load().pww_conv3x3_workspace_bytes(ops.ctypes.byref(d))
            split = nbytes // (4 * rows * S * S * Cout) if nbytes else 1
            tn_auto = 128 if Cout % 128 == 0 else 64
            best = ""
            if args.sweep:
                res = []
                nslab = 9 * Cin // 64
                for tn in (64, 128, 160):
                    if Cout % tn:
                        continue
                    for sk in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32):
                        if sk > nslab // 4:
                            continue
                        res.append((replay_us(lambda: hip(tn, sk)), tn, sk))
                res.sort()
                # the best cell of all, then the best cell of every tile width
                per_width = [min(r for r in res if r[1] == tn) for tn in (64, 128, 160) if any(r[1] == tn for r in res)]
                best = "; ".join(["%.1f us @ %d, %d" % res[0]] + ["%d: %.1f @ %d" % (tn, t, sk) for t, tn, sk in per_width]) if res else ""
            tot.setdefault(rows, [0.0, 0.0])
            tot[rows][0] += count * t_stock
            tot[rows][1] += count * t_hip
            lines.append("| %d | %d->%d | %d | %d | %d | %d | %.1f | %.1f | %.0f (%.0f %%) | %.1f | %.0f (%.0f %%) | %.2f | %d, %d | %.1e | %s |" % (
                rows, Cin, Cout, S, stride, up, count, flop / 1e9, t_stock, flop / t_stock / 1e6, 100 * flop / t_stock / 1e6 / PEAK_TFLOPS,
                t_hip, flop / t_hip / 1e6, 100 * flop / t_hip / 1e6 / PEAK_TFLOPS, t_hip / t_stock, tn_auto, split, err, best))
            print(lines[-1], flush=True)
    for rows, (s, h) in sorted(tot.items()):
        lines.append("")
        lines.append("rows %d: per UNet forward (count-weighted) stock %.0f us, HIP %.0f us (%.2fx)" % (rows, s, h, s / h))
        print(lines[-1])
    text = "\n".join(lines + ([""] + ["| rows | Cin->Cout | out | s | up | stock kernels |", "|---|---|---|---|---|---|"] + kern_lines if kern_lines else []))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
