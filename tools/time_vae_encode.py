#!/usr/bin/env python
"""What the AutoencoderKL encode costs, native against stock (profiles/vae_encode.md).

1. Whole encode, image on the device -> the scaled latent, bf16, SD encoder topology with seeded random weights (sd_standin.AutoencoderKLEncDec),
   for a 512 x 512 and a 512 x 2048 image:
     native          pww_hip.vae_encode.encode(vae, image, noise="sample")
     native uint8    the same from the [1, H, W, 3] uint8 pixels
     stock NCHW      the line PWW_VAE_ENCODE=0 keeps: 0.18215 * vae.encode(image).latent_dist.sample().float()
     stock NHWC      the same with the module and the input in channels_last
   Alternating rounds after a warm-up of every setting (wall time of one call, device synchronised before and after); medians, and the spread
   (max - min) / median of each setting.
2. Each new kernel alone at the encoder's shapes against the stock op sequence it replaces (stream time per call):
     head            pww_vaeenc_head_fwd (both input forms)  vs  conv2d 3 -> 128 + the channels_last copy the next native op needs
     down            pww_vaeenc_down_fwd at the three levels  vs  F.pad + conv2d stride 2
     tail            pww_vaeenc_tail_fwd  vs  group_norm -> silu -> conv2d -> 1 x 1 conv2d -> chunk, clamp, exp, mul, add, scale
3. Parity of that very full-size native run against the fp32 encoder on the same weights, under the rule of the tests (tests/vaeenc_cases.py):
   the tool FAILS above the bar.

    python tools/time_vae_encode.py [--rounds 7] [--dtype bf16|fp16] [--skip-wide] [--kernels-only]
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

import pww_hip  # noqa: E402
import vaeenc_cases as C  # noqa: E402
from pww_hip import vae as V  # noqa: E402
from pww_hip import vae_encode as E  # noqa: E402


def stream_us(f, iters=50):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        f()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stock_latent(vae, x):
    return 0.18215 * vae.encode(x).latent_dist.sample().float()


def whole_encode(vae, vae_cl, shape, dtype, dev, rounds):
    x = C.image(shape, dtype, dev)
    x_cl = x.contiguous(memory_format=torch.channels_last)
    u8 = ((x.float() + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    settings = {"native": lambda: E.encode(vae, x, noise="sample"),
                "native uint8": lambda: E.encode(vae, u8, noise="sample"),
                "stock NCHW": lambda: stock_latent(vae, x),
                "stock NHWC": lambda: stock_latent(vae_cl, x_cl)}
    with torch.no_grad():
        for f in settings.values():     # warm-up: MIOpen's solver lookup, the libraries, the allocator
            f()
            f()
        times = {k: [] for k in settings}
        for _ in range(rounds):
            for k, f in settings.items():
                times[k].append(wall_ms(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("encode %s %s  %-12s median %8.2f ms   spread %.1f %%   (min %.2f, max %.2f, %d rounds)"
              % (tuple(shape), str(dtype)[6:], k, med[k], 100 * (max(v) - min(v)) / med[k], min(v), max(v), len(v)), flush=True)
    best_stock = min(med["stock NCHW"], med["stock NHWC"])
    print("encode %s: native / best stock = %.3f, native uint8 / best stock = %.3f"
          % (tuple(shape), med["native"] / best_stock, med["native uint8"] / best_stock), flush=True)
    return med


def parity(vae, shape, dtype, dev):
    st = C.encode_checks(vae, shape, dtype, dev)      # asserts the bars
    C.assert_native(st, 2, attn=V.attn_enabled(), head=E.head_enabled(), down=E.down_enabled(), tail=E.tail_enabled())
    print("parity %s %s: within the bars, every part but what a switch turned off native" % (tuple(shape), str(dtype)[6:]), flush=True)


def report(what, names, fns, iters):
    pairs = [[stream_us(f, iters) for _ in range(3)] for f in fns]
    med = [statistics.median(p) for p in pairs]
    spread = max((max(p) - min(p)) / statistics.median(p) for p in pairs)
    best = min(med[1:])
    print("%s: %s, ratio to the better stock %.3f, spread %.1f %%"
          % (what, ", ".join("%s %8.1f us" % (n, m) for n, m in zip(names, med)), med[0] / best, 100 * spread), flush=True)


def kernels_alone(vae, dtype, dev, shapes):
    enc = vae.encoder
    g = torch.Generator().manual_seed(11)
    for (_, _, H, W) in shapes:
        x = C.image((1, 3, H, W), dtype, dev)
        u8 = ((x.float() + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        cin = enc.conv_in
        x_cl = x.contiguous(memory_format=torch.channels_last)
        report("head %4d x %4d %s" % (H, W, str(dtype)[6:]), ("pww_vaeenc_head_fwd", "uint8 form", "stock conv2d + channels_last", "stock, channels_last input"),
               (lambda: E.head(x, cin.weight, cin.bias), lambda: E.head(u8, cin.weight, cin.bias), lambda: E.head_stock(x, cin), lambda: E.head_stock(x_cl, cin)), 20)
        h, w = H, W
        for block in enc.down_blocks[:3]:
            conv = block.downsamplers[0].conv
            a = torch.randn(1, conv.in_channels, h, w, generator=g).to(dev, dtype).contiguous(memory_format=torch.channels_last)
            a_nchw = a.contiguous()
            report("down %4d x %4d x %3d %s" % (h, w, conv.in_channels, str(dtype)[6:]), ("pww_vaeenc_down_fwd", "stock pad + conv2d channels_last", "NCHW"),
                   (lambda: E.down(a, conv.weight, conv.bias), lambda: E.down_stock(a, conv), lambda: E.down_stock(a_nchw, conv)), 20)
            h, w = h // 2, w // 2
        a = torch.randn(1, 512, h, w, generator=g).to(dev, dtype).contiguous(memory_format=torch.channels_last)
        a_nchw = a.contiguous()
        n = torch.randn(1, 4, h, w, generator=g).to(dev, dtype)
        norm, conv, qc = enc.conv_norm_out, enc.conv_out, vae.quant_conv
        report("tail %4d x %4d %s" % (h, w, str(dtype)[6:]), ("pww_vaeenc_tail_fwd", "stock ops channels_last", "NCHW"),
               (lambda: E.tail(a, norm.weight, norm.bias, conv.weight, conv.bias, qc.weight, qc.bias, n, norm.eps, moments=False),
                lambda: E.tail_stock(a, norm, conv, qc, n), lambda: E.tail_stock(a_nchw, norm, conv, qc, n)), 50)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--skip-wide", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    dev = torch.device("cuda:0")
    pww_hip.enable_miopen_find()        # what the drop-in API runs under: the stock convolutions get MIOpen's fastest solver
    print("switches: PWW_VAE_ENC_HEAD %s, PWW_VAE_ENC_DOWN %s, PWW_VAE_ENC_TAIL %s, PWW_VAE_ATTN %s (the whole encode runs as they say; the kernels alone "
          "are timed either way)" % tuple("on" if f() else "off" for f in (E.head_enabled, E.down_enabled, E.tail_enabled, V.attn_enabled)), flush=True)
    shapes = [(1, 3, 512, 512)] + ([] if args.skip_wide else [(1, 3, 512, 2048)])
    vae = C.make_vae(dtype, dev)
    vae_cl = C.make_vae(dtype, dev).to(memory_format=torch.channels_last)
    assert E.covers(vae)
    with torch.no_grad():
        kernels_alone(vae, dtype, dev, shapes)
        for shape in ([] if args.kernels_only else shapes):
            whole_encode(vae, vae_cl, shape, dtype, dev, args.rounds)
        if not args.kernels_only:
            parity(vae, shapes[0], dtype, dev)
    print("time_vae_encode OK")


if __name__ == "__main__":
    main()
