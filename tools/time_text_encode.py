#!/usr/bin/env python
"""What the CLIP text encoder costs, native against stock (profiles/text_encoder.md).

Topologies, seeded random weights (sd_standin.CLIPTextEncoder), bf16 unless --dtype says otherwise:
  SD1.5   12 layers, C 768, 12 heads, 3072 inner, quick_gelu          SD2.x   23 layers, C 1024, 16 heads, 4096 inner, gelu

1. Whole encode of R rows of 77 tokens, R = 2 (a plain request), 6 (three chunks), 7 and 14 (five region prompts beside the request's
   cond + uncond, 1 and 2 chunks):
     parent          R calls of the stock module with a [1, 77] batch each: what PWW_TEXT_ENCODE=0 keeps
     stock batched   one call of the stock module with the [R, 77] batch (for orientation: no route here takes it)
     native          pww_hip.text_encode.encode as the defaults route it
     native, GEMMs stock / native, GEMMs forced     PWW_TEXT_LINEAR=0 / force
   Alternating rounds after a warm-up of every setting (wall time of one call, device synchronised before and after: the encode is
   launch-bound, the host's time IS the cost); medians, and the spread (max - min) / median of each setting.
2. Each part alone (stream time per call, three repeats, the spread stated):
     attention       pww_text_attn_fwd  vs  F.scaled_dot_product_attention(is_causal=True)  vs  the eager sequence (two products, mask, softmax)
     act             pww_text_act  vs  the stock expression
     embed           pww_text_embed_ln  vs  embedding + add + layer_norm
     GEMMs           each of the four shapes per topology at M = 154 and M = 1078: the stock GEMM against ops.linear over tile widths and K splits
3. A whole tiny request (paint_with_words, tiny UNet, a CLIPTextEncoder of its width) with and without the route.

    python tools/time_text_encode.py [--rounds 9] [--dtype bf16|fp16] [--skip-sd2] [--parts-only] [--no-sweep]
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
import torch.nn.functional as F  # noqa: E402

import pww_hip  # noqa: E402,F401
import text_cases as tc  # noqa: E402
from pww_hip import ops  # noqa: E402
from pww_hip import text_encode as E  # noqa: E402
from sd_standin import CLIPTextEncoder  # noqa: E402

TOPOLOGIES = {"SD1.5": dict(ctx_dim=768, layers=12, heads=12, intermediate=3072, hidden_act="quick_gelu"),
              "SD2.x": dict(ctx_dim=1024, layers=23, heads=16, intermediate=4096, hidden_act="gelu")}
ROWS = (2, 6, 7, 14)


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


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def under(f, **kw):
    def g():
        with env(**kw):
            return f()
    return g


def whole_encode(name, module, R, rounds):
    dev = module.final_layer_norm.weight.device
    ids = tc.prompt_ids(R)
    ids_dev = ids.to(dev)
    settings = {"parent": lambda: E.encode_stock(module, ids_dev),
                "stock batched": lambda: module(ids_dev)[0],
                "native": lambda: E.encode(module, ids),
                "native, GEMMs stock": under(lambda: E.encode(module, ids), PWW_TEXT_LINEAR="0"),
                "native, GEMMs forced": under(lambda: E.encode(module, ids), PWW_TEXT_LINEAR="force")}
    with torch.no_grad():
        for f in settings.values():
            f()
            f()
        times = {k: [] for k in settings}
        for _ in range(rounds):
            for k, f in settings.items():
                times[k].append(wall_ms(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("encode %s R %2d  %-22s median %7.3f ms   spread %5.1f %%   (min %.3f, max %.3f, %d rounds)   / parent %.3f"
              % (name, R, k, med[k], 100 * (max(v) - min(v)) / med[k], min(v), max(v), len(v), med[k] / med["parent"]), flush=True)
    return med


def report(what, names, fns, iters=50):
    reps = [[stream_us(f, iters) for _ in range(3)] for f in fns]
    med = [statistics.median(p) for p in reps]
    spread = max((max(p) - min(p)) / statistics.median(p) for p in reps)
    print("%s: %s, ratio to the better stock %.3f, spread %.1f %%"
          % (what, ", ".join("%s %7.1f us" % (n, m) for n, m in zip(names, med)), med[0] / min(med[1:]), 100 * spread), flush=True)
    return med


def parts_alone(name, cfg, dtype, dev, sweep):
    C, H, inner, act = cfg["ctx_dim"], cfg["heads"], cfg["intermediate"], cfg["hidden_act"]
    g = torch.Generator().manual_seed(3)
    for R in (2, 14):
        qkv = torch.randn(R, 77, 3 * C, generator=g).to(dev, dtype)
        q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(R, 77, H, 64).transpose(1, 2) for i in range(3))
        report("attention %s R %2d" % (name, R), ("pww_text_attn_fwd", "SDPA is_causal (+ merge)", "eager sequence"),
               (lambda: E.attention(qkv, H), lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(R, 77, C),
                lambda: E.attention_stock(qkv, H)))
        f = torch.randn(R * 77, inner, generator=g).to(dev, dtype)
        report("act %s %s R %2d" % (act, name, R), ("pww_text_act", "stock expression"), (lambda: E.act_(f, act), lambda: E.act_stock(f, act)))
        tok, pos = torch.randn(49408, C, generator=g).to(dev, dtype), torch.randn(77, C, generator=g).to(dev, dtype)
        w, b = torch.ones(C, device=dev, dtype=dtype), torch.zeros(C, device=dev, dtype=dtype)
        ids = tc.prompt_ids(R).to(dev)
        ids32 = ids.to(torch.int32)
        report("embed %s R %2d" % (name, R), ("pww_text_embed_ln", "embedding + add + layer_norm"),
               (lambda: E.embed_ln(ids32, tok, pos, w, b, 1e-5), lambda: E.embed_ln_stock(ids, tok, pos, w, b, 1e-5)))
        del tok
    if not sweep:
        return
    for K, N, what in ((C, 3 * C, "qkv"), (C, C, "out_proj"), (C, inner, "fc1"), (inner, C, "fc2 + residual")):
        wt, bias = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev, dtype), torch.randn(N, generator=g).to(dev, dtype)
        for M in (154, 1078):
            x = torch.randn(M, K, generator=g).to(dev, dtype)
            res = torch.randn(M, N, generator=g).to(dev, dtype) if what.startswith("fc2") else None
            stock = (lambda: F.linear(x, wt, bias) + res) if res is not None else (lambda: F.linear(x, wt, bias))
            t_stock = statistics.median(stream_us(stock) for _ in range(3))
            rows = []
            for tile_n in (64, 128):
                for splitk in (1, 2, 3, 4, 6, 8):
                    if N % tile_n or splitk > K // 64:
                        continue
                    t = statistics.median(stream_us(lambda: ops.linear(x, wt, bias, residual=res, tile_n=tile_n, splitk=splitk)) for _ in range(3))
                    rows.append((t, tile_n, splitk))
            t_def = statistics.median(stream_us(lambda: ops.linear(x, wt, bias, residual=res, tile_n=E._gemm_plan(K, N)[0], splitk=E._gemm_plan(K, N)[1])) for _ in range(3))
            best = min(rows)
            print("gemm %s %-14s K %4d N %4d M %4d: stock %6.1f us | ops.linear as routed (%d, %d) %6.1f us | best (%d, %d) %6.1f us | all: %s"
                  % (name, what, K, N, M, t_stock, *E._gemm_plan(K, N), t_def, best[1], best[2], best[0],
                     " ".join("(%d,%d) %.1f" % (tn, sk, t) for t, tn, sk in rows)), flush=True)


def tiny_request(dtype, dev, rounds):
    from PIL import Image
    import paint_with_words as pw
    import pww_cases as cases
    vae, unet, tiny_text, tok, sch = cases.build_tools("tiny", dtype=dtype, device=dev)
    clip = CLIPTextEncoder(ctx_dim=tiny_text.pos.shape[1], layers=12, heads=1, intermediate=256, seed=9).to(device=dev, dtype=dtype)
    img = Image.fromarray(cases.load_example_rgb())

    def run():
        return pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=img, input_prompt=cases.RUNNER_PROMPT, num_inference_steps=3,
                                   guidance_scale=7.5, seed=3, device=str(dev), weight_function=cases.weight_fn_runner,
                                   preloaded_utils=(vae, unet, clip, tok, sch), return_latents=True)
    settings = {"route on": run, "PWW_TEXT_ENCODE=0": under(run, PWW_TEXT_ENCODE="0")}
    for f in settings.values():
        f()
        f()
    times = {k: [] for k in settings}
    for _ in range(rounds):
        for k, f in settings.items():
            times[k].append(wall_ms(f))
    for k, v in times.items():
        m = statistics.median(v)
        print("tiny request (3 steps, 12-layer one-head text encoder) %-18s median %8.2f ms   spread %5.1f %%" % (k, m, 100 * (max(v) - min(v)) / m), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp16"))
    ap.add_argument("--skip-sd2", action="store_true")
    ap.add_argument("--parts-only", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    dev = torch.device("cuda:0")
    print("switches: PWW_TEXT_ENCODE %s, PWW_TEXT_EMBED %s, PWW_TEXT_ATTN %s, PWW_TEXT_ACT %s, PWW_TEXT_LINEAR %s; LINEAR_ROUTES %s"
          % (*("on" if f() else "off" for f in (E.enabled, E.embed_enabled, E.attn_enabled, E.act_enabled)), E.linear_mode(), dict(E.LINEAR_ROUTES)), flush=True)
    with torch.no_grad():
        for name, cfg in TOPOLOGIES.items():
            if name == "SD2.x" and args.skip_sd2:
                continue
            parts_alone(name, cfg, dtype, dev, not args.no_sweep)
            if args.parts_only:
                continue
            module = CLIPTextEncoder(**cfg).to(device=dev, dtype=dtype).eval()
            assert E.covers(module)
            ids = tc.prompt_ids(2)
            stock = module(ids.to(dev))[0].float()
            err = (E.encode(module, ids).float() - stock).abs().max().item() / stock.abs().max().item()
            print("encode %s: native against the stock module, max abs / max|out| = %.3e" % (name, err), flush=True)
            for R in ROWS:
                whole_encode(name, module, R, args.rounds)
            del module
        if not args.parts_only:
            tiny_request(dtype, dev, args.rounds)
    print("time_text_encode OK")


if __name__ == "__main__":
    main()
