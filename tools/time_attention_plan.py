"""Host cost of one call of the attention plug (pww_hip.attention._attention) with every ops launch replaced by a stand-in that returns a
ready tensor: what is left is the plug's own Python plus the CPU GEMMs of a C = 64, N = 16 layer. No GPU, no library.

    python tools/time_attention_plan.py [--against DIR] [--calls 100] [--rounds 400]

Without --against: this checkout's package alone. With it: DIR holds a second pww_hip package (another checkout's paint-with-words-sd_amd); both
are loaded into this process and timed in alternating bursts of --calls calls, the order swapped every round, so that what disturbs the
machine disturbs both. Prints one JSON line per case: per package the median and the fastest burst in microseconds per call, and with --against
the median and the quartiles of the paired differences (this checkout minus DIR).
Cases: `dict_max` (dict context, 0.3 * w * log(1 + sigma) * qk.max(): the symbolic-statistic plan, qk_parts route) and `self` (context None)."""
import argparse
import importlib.util
import json
import math
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, D, N, M, B = 64, 32, 16, 77, 2


class FakeCuda(torch.Tensor):
    is_cuda = True


def load(name, root):
    """(attention, ops) of the pww_hip package under `root`, imported under the module name `name`, its launches replaced."""
    init = os.path.join(root, "pww_hip", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, init, submodule_search_locations=[os.path.dirname(init)])
    sys.modules[name] = module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    attention, ops = sys.modules[name + ".attention"], sys.modules[name + ".ops"]
    out, parts = torch.zeros(B, N, C, dtype=torch.float16), torch.zeros(B, 3, 4, dtype=torch.float64)
    ops.attention = lambda *a, **kw: out
    ops.qk_parts = lambda *a, **kw: parts
    attention.QPROJ_STAT, attention.FUSED_CROSS = "0", False
    return attention


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=400)
    args = ap.parse_args()
    here = os.path.join(REPO, "paint-with-words-sd_amd")
    sys.path.insert(0, here)       # sd_standin
    from sd_standin import CrossAttention
    packages = {"this": load("pww_hip_this", here)}
    if args.against:
        packages["other"] = load("pww_hip_other", args.against)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    hidden = torch.randn(B, N, C).half().as_subclass(FakeCuda)
    cross, self_attn = CrossAttention(C, 32, C // D, D).half(), CrossAttention(C, None, C // D, D).half()
    contexts = {name: {"CONTEXT_TENSOR": torch.randn(B, M, 32).half(), "CROSS_ATTENTION_WEIGHT_%d" % N: torch.rand(N, M), "SIGMA": 3.0,
                       "WEIGHT_FUNCTION": lambda w, sigma, qk: 0.3 * w * math.log(1 + sigma) * qk.max(), attention.KV_CACHE: {}}
                for name, attention in packages.items()}

    def burst(name, case):
        mod, context = (cross, contexts[name]) if case == "dict_max" else (self_attn, None)
        call = packages[name]._attention
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call(mod, hidden, context, None)
        return (time.perf_counter() - t0) / args.calls * 1e6

    for case in ("dict_max", "self"):
        times, diffs = {name: [] for name in packages}, []
        for r in range(args.rounds + 10):
            order = list(packages) if r % 2 == 0 else list(packages)[::-1]
            t = {name: burst(name, case) for name in order}
            if r >= 10:         # the first rounds warm the caches
                for name in t:
                    times[name].append(t[name])
                if args.against:
                    diffs.append(t["this"] - t["other"])
        line = {"case": case, "calls": args.calls, "rounds": args.rounds}
        for name, v in times.items():
            line[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)}
        if diffs:
            line["this_minus_other_us"] = {"median": round(statistics.median(diffs), 2), "quartiles": [round(x, 2) for x in statistics.quantiles(diffs, n=4)]}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
