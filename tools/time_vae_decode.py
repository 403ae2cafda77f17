#!/usr/bin/env python
"""What the AutoencoderKL decode costs, native against stock (profiles/vae_decode.md).

1. Whole decode, latent -> the [B, H, W, 3] uint8 image ON THE HOST (what `_pil_from_latents` hands to PIL), bf16, SD decoder topology with
   seeded random weights, for a [1, 4, 64, 64] and a [1, 4, 64, 256] latent:
     native          pww_hip.vae.decode(vae, z, "uint8").cpu()
     stock NCHW      the code `PWW_VAE=0` keeps: vae.decode(z).sample, float post-processing and the float image copied to the host
     stock NHWC      the same with the module and the input in channels_last
   Alternating rounds after a warm-up of every setting; medians, and the spread (max - min) / median of each setting.
2. Each new kernel alone at the decoder's shapes against the stock op sequence it replaces (stream time per call):
     attention       pww_vae_attn_fwd on the slices of one [1, N, 1536] tensor  vs  scaled bmm -> fp32 softmax -> bmm
     tail            pww_vae_tail_fwd (uint8 form)  vs  group_norm -> silu -> conv2d -> / 2 + 0.5, clamp, float, permute, * 255, round, uint8
3. Parity of that very full-size native run against the fp32 decoder on the same weights, under the rule of the tests (tests/vae_cases.py):
   the tool FAILS above the bar.

    python tools/time_vae_decode.py [--rounds 7] [--dtype bf16|fp16] [--skip-wide]
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
import vae_cases as C  # noqa: E402
from pww_hip import vae as V  # noqa: E402


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
    f()                     # (ends in a copy to the host: synchronous)
    return (time.perf_counter() - t0) * 1e3


def stock_image(vae, z):
    """The stock lines of _pil_from_latents: the float image goes to the host, the 8-bit rounding happens there."""
    decoded = vae.decode(z).sample
    pixels = (decoded / 2 + 0.5).clamp(0, 1).detach().float().cpu().permute(0, 2, 3, 1).numpy()
    return (pixels * 255).round().astype("uint8")


def whole_decode(vae, vae_cl, shape, dtype, dev, rounds):
    z = C.latent(shape, dtype, dev)
    z_cl = z.contiguous(memory_format=torch.channels_last)
    settings = {"native": lambda: V.decode(vae, z, "uint8").cpu().numpy(),
                "stock NCHW": lambda: stock_image(vae, z),
                "stock NHWC": lambda: stock_image(vae_cl, z_cl)}
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
        print("decode %s %s  %-11s median %8.2f ms   spread %.1f %%   (min %.2f, max %.2f, %d rounds)"
              % (tuple(shape), str(dtype)[6:], k, med[k], 100 * (max(v) - min(v)) / med[k], min(v), max(v), len(v)), flush=True)
    best_stock = min(med["stock NCHW"], med["stock NHWC"])
    print("decode %s: native / best stock = %.3f" % (tuple(shape), med["native"] / best_stock), flush=True)
    return med


def parity(vae, shape, dtype, dev):
    st = C.decode_checks(vae, shape, dtype, dev)      # asserts the bars
    C.assert_native(st, 2, attn=V.attn_enabled(), tail=V.tail_enabled())
    print("parity %s %s: within the bar, every part but what a switch turned off native" % (tuple(shape), str(dtype)[6:]), flush=True)


def kernels_alone(vae, dtype, dev, shapes):
    dec = vae.decoder
    g = torch.Generator().manual_seed(11)
    for (_, _, h, w) in shapes:
        N = h * w
        qkv = torch.randn(1, N, 1536, generator=g).to(dev, dtype)
        q, k, v = qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:]
        pairs = [stream_us(lambda: V.attention(q, k, v)) for _ in range(3)], [stream_us(lambda: V.attention_stock(q, k, v)) for _ in range(3)]
        ours, theirs = (statistics.median(p) for p in pairs)
        spread = max((max(p) - min(p)) / statistics.median(p) for p in pairs)
        print("attention N %5d %s: pww_vae_attn_fwd %8.1f us, stock bmm / softmax / bmm %8.1f us, ratio %.3f, spread %.1f %%"
              % (N, str(dtype)[6:], ours, theirs, ours / theirs, 100 * spread), flush=True)
        x = torch.randn(1, 128, 8 * h, 8 * w, generator=g).to(dev, dtype).contiguous(memory_format=torch.channels_last)
        norm, conv = dec.conv_norm_out, dec.conv_out
        native = lambda: V.tail(x, norm.weight, norm.bias, conv.weight, conv.bias, norm.eps, "uint8")      # noqa: E731
        stock = lambda: V.tail_stock(x, norm, conv, "uint8")                                              # noqa: E731
        stock_nchw = lambda xn=x.contiguous(): V.tail_stock(xn, norm, conv, "uint8")                      # noqa: E731
        pairs = [[stream_us(f, 20) for _ in range(3)] for f in (native, stock, stock_nchw)]
        a, b, c = (statistics.median(p) for p in pairs)
        spread = max((max(p) - min(p)) / statistics.median(p) for p in pairs)
        print("tail %4d x %4d %s: pww_vae_tail_fwd %8.1f us, stock ops channels_last %8.1f us, NCHW %8.1f us, ratio to the better %.3f, spread %.1f %%"
              % (8 * h, 8 * w, str(dtype)[6:], a, b, c, a / min(b, c), 100 * spread), flush=True)


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
    print("switches: PWW_VAE_ATTN %s, PWW_VAE_TAIL %s (the whole decode runs as they say; the kernels alone are timed either way)"
          % ("on" if V.attn_enabled() else "off", "on" if V.tail_enabled() else "off"), flush=True)
    shapes = [(1, 4, 64, 64)] + ([] if args.skip_wide else [(1, 4, 64, 256)])
    vae = C.make_vae(dtype, dev)
    vae_cl = C.make_vae(dtype, dev).to(memory_format=torch.channels_last)
    assert V.covers(vae)
    with torch.no_grad():
        kernels_alone(vae, dtype, dev, shapes)
        for shape in ([] if args.kernels_only else shapes):
            whole_decode(vae, vae_cl, shape, dtype, dev, args.rounds)
        if not args.kernels_only:
            parity(vae, shapes[0], dtype, dev)
    print("time_vae_decode OK")


if __name__ == "__main__":
    main()
