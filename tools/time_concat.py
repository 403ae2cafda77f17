#!/usr/bin/env python
"""Per-shape timing of the two readers of `torch.cat([x, skip], 1)` in the SD1.5 UNet's twelve up-block ResnetBlock2D at 2 rows: the stock
sequence (torch.cat, then ops.group_norm with SiLU on the concatenation, then ops.conv3x3_shortcut reading it again) against the two-source
pair (ops.group_norm_cat, ops.conv3x3_shortcut_cat: csrc/pww_concat.hip), which never makes the tensor. conv1 and norm2, which sit between
the two readers and do not touch the concatenation, are left out of both. Every call is captured once and replayed 20x back to back from a
hipGraph, best of 5 (event interval / 20: includes the dispatch gaps, no host in the loop). Also checks that the pair's results equal the
stock sequence's bit for bit.

Usage: python tools/time_concat.py [--sweep] [--dtype bf16] [out.md]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from time_convtail import SPLITS, replay_us  # noqa: E402

# (C1 = the running tensor's channels, C2 = the skip's, Cout, size, count per forward) at 512 x 512 (latent 64 x 64)
SHAPES = [(1280, 1280, 1280, 8, 3), (1280, 1280, 1280, 16, 2), (1280, 640, 1280, 16, 1),
          (1280, 640, 640, 32, 1), (640, 640, 640, 32, 1), (640, 320, 640, 32, 1),
          (640, 320, 320, 64, 1), (320, 320, 320, 64, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--sweep", action="store_true", help="also time the two-source tail at tile_n 64 / 128 / 160 and a range of K splits")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    import pww_hip
    from pww_hip import ops
    pww_hip.load_library()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    cl = torch.channels_last
    rows = args.rows
    lines = ["| rows | C1 + C2 -> Cout | size | n/fwd | cat us | GN(cat) us | convtail(cat) us | stock us | GN two-source us | convtail two-source us | pair us | pair / stock | saved us | equal |"
             + (" best cell per tile width | sweep (tile / split: us) |" if args.sweep else ""),
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|" + ("---|---|" if args.sweep else "")]
    tot = [0.0, 0.0, 0.0]
    torch.manual_seed(0)
    for C1, C2, Cout, S, count in SHAPES:
        C = C1 + C2
        x1 = torch.randn(rows, C1, S, S, device=dev).to(dt).contiguous(memory_format=cl)
        x2 = torch.randn(rows, C2, S, S, device=dev).to(dt).contiguous(memory_format=cl)
        h = torch.randn(rows, Cout, S, S, device=dev).to(dt).contiguous(memory_format=cl)
        gamma, beta = (1 + 0.1 * torch.randn(C, device=dev)).to(dt), (0.1 * torch.randn(C, device=dev)).to(dt)
        w = (torch.randn(Cout, Cout, 3, 3, device=dev) / (3 * Cout ** 0.5)).to(dt).contiguous(memory_format=cl)
        wsc = (torch.randn(Cout, C, 1, 1, device=dev) / C ** 0.5).to(dt)
        b, bsc = (torch.randn(Cout, device=dev) * 0.1).to(dt), (torch.randn(Cout, device=dev) * 0.1).to(dt)
        cat = torch.cat([x1, x2], dim=1)

        def stock():
            c = torch.cat([x1, x2], dim=1)
            return ops.group_norm(c, 32, gamma, beta, 1e-5, act="silu"), ops.conv3x3_shortcut(h, w, b, c, wsc, bsc)

        def pair():
            return ops.group_norm_cat(x1, x2, 32, gamma, beta, 1e-5, act="silu"), ops.conv3x3_shortcut_cat(h, w, b, x1, x2, wsc, bsc)
        equal = all(torch.equal(a, c) for a, c in zip(stock(), pair()))
        t_cat = replay_us(lambda: torch.cat([x1, x2], dim=1))
        t_gn = replay_us(lambda: ops.group_norm(cat, 32, gamma, beta, 1e-5, act="silu"))
        t_tail = replay_us(lambda: ops.conv3x3_shortcut(h, w, b, cat, wsc, bsc))
        t_gn2 = replay_us(lambda: ops.group_norm_cat(x1, x2, 32, gamma, beta, 1e-5, act="silu"))
        t_tail2 = replay_us(lambda: ops.conv3x3_shortcut_cat(h, w, b, x1, x2, wsc, bsc))
        t_stock, t_pair = replay_us(stock), replay_us(pair)
        tot[0] += count * t_cat
        tot[1] += count * t_stock
        tot[2] += count * t_pair
        cells = ""
        if args.sweep:          # the two-source tail alone at every tile width that divides Cout and a range of K splits (time_convtail.py's grid)
            res = []
            nslab = (9 * Cout + C) // 64
            for tn in (64, 128, 160):
                if Cout % tn:
                    continue
                for sk in SPLITS:
                    if sk > nslab // 4 or rows * S * S * Cout * sk * 4 > 1 << 28:
                        continue
                    res.append((replay_us(lambda: ops.conv3x3_shortcut_cat(h, w, b, x1, x2, wsc, bsc, tile_n=tn, splitk=sk)), tn, sk))
            per_width = [min(r for r in res if r[1] == tn) for tn in (64, 128, 160) if any(r[1] == tn for r in res)]
            cells = " " + "; ".join("%d: %.1f @ %d" % (tn, t, sk) for t, tn, sk in per_width) + " | " + " ".join("%d/%d:%.1f" % (tn, sk, t) for t, tn, sk in res) + " |"
        lines.append("| %d | %d + %d -> %d | %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f | %s |%s" % (
            rows, C1, C2, Cout, S, count, t_cat, t_gn, t_tail, t_stock, t_gn2, t_tail2, t_pair, t_pair / t_stock, t_stock - t_pair, "yes" if equal else "NO",
            cells))
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("rows %d: per UNet forward (count-weighted) torch.cat %.0f us, stock sequence %.0f us, two-source pair %.0f us (%.0f us less)"
                 % (rows, tot[0], tot[1], tot[2], tot[1] - tot[2]))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
