#!/usr/bin/env python
"""Per-shape timing of the SD1.5 UNet's feed-forward and proj_out GEMMs at 2 rows (bf16): the stock sequence (F.linear -> hipBLASLt, then
ops.geglu, or then the residual add) against ops.linear (csrc/pww_linear.hip) with the post-op in the GEMM's epilogue, at the library's
tile / split choice and, with --sweep, over tile_n x split. Every call is captured once and replayed 20x back to back from a hipGraph (event
interval / 20: includes the dispatch gaps, no host in the loop). Each HIP result is also checked against the stock sequence's
(max |diff| / max |ref|). The route table of pww_hip/blocks.py (LINEAR_ROUTES) and the tile table of csrc/pww_linear.hip (LIN_TUNED) are
read off the grid this prints.

Usage: python tools/time_linear.py [--rows 2,16] [--sweep] [--dtype bf16] [out.md]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_TFLOPS = 2500.0          # dense bf16 / fp16 MFMA peak of the MI355X
# (tokens per row, K, N, epilogue, count per forward) of the SD1.5 UNet at 512 x 512: GEGLU projection, feed-forward output, proj_out
SHAPES = [(4096, 320, 2560, "geglu", 5), (4096, 1280, 320, "residual", 5), (4096, 320, 320, "residual", 5),
          (1024, 640, 5120, "geglu", 5), (1024, 2560, 640, "residual", 5), (1024, 640, 640, "residual", 5),
          (256, 1280, 10240, "geglu", 5), (256, 5120, 1280, "residual", 5), (256, 1280, 1280, "residual", 5),
          (64, 1280, 10240, "geglu", 1), (64, 5120, 1280, "residual", 1), (64, 1280, 1280, "residual", 1)]


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
    ap.add_argument("--rows", default="2")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--sweep", action="store_true", help="also time tile_n 64 / 128 over a range of K splits")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    from pww_hip import ops, _lib
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    lines = ["| rows | M | K | N | epilogue | n/fwd | GFLOP | stock us (GEMM + post-op) | stock GEMM alone us | HIP us | HIP TF/s (%peak) | HIP/stock | tile_n, split | diff | best sweep | sweep grid (tile_n: split=us) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    tot = {}
    torch.manual_seed(0)
    for rows in [int(r) for r in args.rows.split(",")]:
        for tok, K, N, epi, count in SHAPES:
            M = rows * tok
            x = torch.randn(M, K, device=dev).to(dt)
            w = (torch.randn(N, K, device=dev) / K ** 0.5).to(dt)
            b = (torch.randn(N, device=dev) * 0.1).to(dt)
            r = torch.randn(M, N, device=dev).to(dt) if epi == "residual" else None
            flop = 2.0 * M * N * K
            if epi == "geglu":
                stock = lambda: ops.geglu(F.linear(x, w, b))  # noqa: E731
                hip = lambda tn=0, sk=0: ops.linear(x, w, b, geglu=True, tile_n=tn, splitk=sk)  # noqa: E731
            else:
                stock = lambda: F.linear(x, w, b) + r  # noqa: E731
                hip = lambda tn=0, sk=0: ops.linear(x, w, b, residual=r, tile_n=tn, splitk=sk)  # noqa: E731
            ref = stock().float()
            diff = ((hip().float() - ref).abs().max() / ref.abs().max()).item()
            t_stock = replay_us(stock)
            t_gemm = replay_us(lambda: F.linear(x, w, b))
            t_hip = replay_us(hip)
            d = _lib.LinearDesc(ops.ctypes.sizeof(_lib.LinearDesc), ops._DT[dt], M, N, K, 3 if epi == "geglu" else 2, 0, 0, 0, 0, 0)
            nbytes = _lib.load_linear().pww_linear_workspace_bytes(ops.ctypes.byref(d))
            split = nbytes // (4 * M * N) if nbytes else 1
            best, grid = "", ""
            if args.sweep:
                res, cells = [], {}
                for tn in (64, 128):
                    if N % tn:
                        continue
                    for sk in (1, 2, 3, 4, 5, 8, 10, 16, 20):
                        if sk > K // 64 // 2 and sk > 1:
                            continue
                        t = replay_us(lambda: hip(tn, sk))
                        res.append((t, tn, sk))
                        cells.setdefault(tn, []).append("%d=%.1f" % (sk, t))
                res.sort()
                best = "%.1f us @ %d, %d" % res[0]
                grid = "; ".join("%d: %s" % (tn, " ".join(v)) for tn, v in cells.items())
            tot.setdefault(rows, [0.0, 0.0])
            tot[rows][0] += count * t_stock
            tot[rows][1] += count * t_hip
            lines.append("| %d | %d | %d | %d | %s | %d | %.1f | %.1f | %.1f | %.1f | %.0f (%.0f %%) | %.2f | auto, %d | %.1e | %s | %s |" % (
                rows, M, K, N, epi, count, flop / 1e9, t_stock, t_gemm, t_hip, flop / t_hip / 1e6, 100 * flop / t_hip / 1e6 / PEAK_TFLOPS,
                t_hip / t_stock, split, diff, best, grid))
            print(lines[-1], flush=True)
    for rows, (s, h) in sorted(tot.items()):
        lines.append("")
        lines.append("rows %d: per UNet forward (count-weighted) stock %.0f us, HIP %.0f us (%.2fx)" % (rows, s, h, s / h))
        print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
