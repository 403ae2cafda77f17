"""The attention plug's plan as a table: for every case of attn_plan_cases.py, attention._attention (or _attention_and_out) runs on the CPU
with every ops launch replaced by a recording stand-in, and the record -- the ordered launches with their arguments, the `projected` flag, the
hipGraph slots, the context's caches, the warning keys -- is compared with the literal in attn_plan_expected.py. No GPU, no library.

In a record a tensor reads `dtype[shape]@name`: `@hidden`, `@map`, `@gate` ... are the case's own tensors, `@qk_parts.out` what a stand-in returned,
`@#3` the third tensor the plug made itself, and `@x.view+64` a view of x at storage offset 64 (key and value of a fused K|V projection are two
views of one tensor). The same name in two places is the same tensor.

`python tests/test_attention_plan_host.py` prints the table as attn_plan_expected.py holds it."""
import inspect
import os
import pprint
import sys

import pytest
import torch

import pww_cases  # noqa: F401  (puts the package on sys.path)
from attn_plan_cases import CASES, DEFAULT, FUNCTIONS, SWITCHES

_DT = {"f16": torch.float16, "f32": torch.float32}
_OPS = ("attention", "attention_scoped", "attention_out", "attention_out_supported", "attention_probs", "qk_parts", "long_qk_parts",
        "scope_head_parts", "scoped_available", "qproj_parts", "qproj_stat", "qk_stats", "resize_tokens", "lora_update")


class FakeCuda(torch.Tensor):
    is_cuda = True


class _Lora:
    """Stands for lora.LoraLayer: the stand-in of ops.lora_update records which projections' stack it was handed."""
    state = "lora-state"

    def stack(self, names):
        return "stack" + repr(names)


class _Names:
    """Names of the tensors of one case, by identity."""

    def __init__(self):
        self.names, self.keep, self.made = {}, [], 0

    def add(self, t, name):
        if torch.is_tensor(t):
            taken = sum(1 for n in self.names.values() if n == name or n.startswith(name + "~"))
            self.names[id(t)] = name if not taken else "%s~%d" % (name, taken + 1)
            self.keep.append(t)
        return t

    def of(self, t):
        if id(t) in self.names:
            return self.names[id(t)]
        base = t._base
        if base is not None:
            return "%s.view+%d" % (self.of(base), t.storage_offset())
        self.made += 1
        self.add(t, "#%d" % self.made)
        return self.names[id(t)]

    def show(self, v):
        if torch.is_tensor(v):
            return "%s%s@%s" % (str(v.dtype).replace("torch.", ""), list(v.shape), self.of(v))
        if isinstance(v, float):
            return float("%.6g" % v)
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, (tuple, list)):
            return tuple(self.show(x) for x in v)
        return type(v).__name__


def _context(spec, names, attention):
    B, N, M = spec["B"], spec["N"], spec["M"]
    g = torch.Generator().manual_seed(1)
    dt = _DT[spec["ctx_dtype"] or spec["dtype"]]
    tensor = names.add(torch.randn(spec["ctxB"] or B, M, spec["Cctx"], generator=g).to(dt), "context")
    if spec["ctx"] != "dict":
        return tensor
    ctx = {"CONTEXT_TENSOR": tensor, "WEIGHT_FUNCTION": FUNCTIONS[spec["f"]], "SIGMA": torch.tensor(3.0) if spec["sigma"] == "tensor" else 3.0}
    kind = spec["map"]
    if kind in ("level", "compact"):
        ctx["CROSS_ATTENTION_WEIGHT_%d" % N] = names.add(torch.rand(N, M, generator=g), "map")
    elif kind == "orig0":
        ctx["CROSS_ATTENTION_WEIGHT_ORIG"] = 0
    else:
        shape = (B, 8, 8, M) if kind == "orig4" else (8, 8, M)
        ctx["CROSS_ATTENTION_WEIGHT_ORIG"] = names.add(torch.rand(*shape, generator=g), "orig")
    if kind in ("compact", "compact_other"):
        ctx[attention.COMPACT_W + str(N)] = names.add(torch.rand(N, 4, generator=g), "compact_w")
        ctx[attention.COMPACT_IDX] = names.add(torch.arange(4, dtype=torch.int32), "compact_idx")
    if spec["bias_cols"] is not None:
        ctx[attention.BIAS_COLS] = spec["bias_cols"]
    if spec["gate"] is not None:
        negative = spec["gate"] == "negative"
        ctx[attention.ROW_GATE] = names.add(torch.tensor([1.0] + [0.5 if negative else 0.0] * (B - 1)), "gate")
        if spec["gate"] != "rows":
            ctx[attention.GATED_ROWS] = 0 if negative else 1
        if negative:
            ctx[attention.COND_ROWS] = 1
    ctx[attention.KV_CACHE] = {}
    if spec["slots"] is not None:
        slots = ctx[attention.COEFF_SLOTS] = attention.CoeffSlots("cpu")
        slots.unsupported = spec["slots"] == "unsupported"
        names.add(slots.dev, "slots")
    if spec["rec"] is not None:
        from pww_hip.attnmaps import AttentionRecorder
        rec = ctx[attention.ATTN_RECORDER] = AttentionRecorder()
        rec.muted = spec["rec"] == "muted"
    return ctx


def _stand_ins(spec, names, log, ops):
    """name -> stand-in of every ops launch the plug can reach: records the call in the last list of `log`, returns tensors of the right shape
    and dtype."""
    def out_like_q(q, *a, **kw):
        return torch.zeros(q.shape, dtype=q.dtype)

    def parts(q, k, heads, kind, **kw):
        return torch.zeros((q.shape[0], 3, 4), dtype=torch.float64)

    def qproj_stat(x, weight, k, heads, kind, gate=None):
        return torch.zeros((x.shape[0], x.shape[1], weight.shape[0]), dtype=x.dtype), torch.zeros((x.shape[0], 3, 4), dtype=torch.float64)

    returns = {
        "attention": out_like_q, "attention_scoped": out_like_q, "attention_out": out_like_q,
        "attention_out_supported": lambda *a, **kw: spec["out_supported"],
        "attention_probs": lambda *a, **kw: kw["out"],
        "qk_parts": parts, "long_qk_parts": parts,
        "scope_head_parts": lambda q, k, heads, kind, **kw: torch.zeros((q.shape[0], heads, 3, 4), dtype=torch.float64),
        "scoped_available": lambda: spec["scoped_lib"],
        "qproj_parts": lambda *a: 3 if spec["qproj_ok"] else 0,
        "qproj_stat": qproj_stat,
        "qk_stats": lambda q, k, heads: torch.tensor([[2.0, -1.0, 3.0, 50.0]] * q.shape[0], dtype=torch.float64),
        "resize_tokens": lambda w_orig, n_tokens: torch.zeros((n_tokens, w_orig.shape[-1]), dtype=torch.float32),
        "lora_update": lambda y, *a: y,
    }

    def make(name):
        sig = inspect.signature(getattr(ops, name))

        def stand_in(*a, **kw):
            bound = sig.bind(*a, **kw).arguments
            log[-1].append((name, {k: names.show(v) for k, v in bound.items()}))
            res = returns[name](*a, **kw)
            for i, t in enumerate(res if isinstance(res, tuple) else (res,)):
                if torch.is_tensor(t) and id(t) not in names.names:
                    names.add(t, "%s.out%s" % (name, i if isinstance(res, tuple) else ""))
            return res
        return stand_in
    return {name: make(name) for name in _OPS}


def record(name):
    """Run one case and return its record."""
    from pww_hip import attention, ops
    from sd_standin import CrossAttention
    spec = dict(DEFAULT, **CASES[name])
    names, warns, runs, undo = _Names(), [], [], []

    def patch(obj, attr, value):
        undo.append((obj, attr, getattr(obj, attr)))
        setattr(obj, attr, value)

    try:
        for sw, value in dict(SWITCHES, **spec["sw"]).items():
            patch(attention, sw, value)
        patch(attention, "_warn_once", lambda key, msg: warns.append(key))
        patch(torch.cuda, "is_current_stream_capturing", lambda: False)
        torch.manual_seed(0)
        C, dt = spec["C"], _DT[spec["dtype"]]
        mod = CrossAttention(C, None if spec["ctx"] == "none" else spec["Cctx"], C // spec["D"], spec["D"])
        for proj in spec["bias_on"]:
            lin = getattr(mod, proj)
            setattr(mod, proj, torch.nn.Linear(lin.in_features, lin.out_features, bias=True))
        mod = mod.to(dt)
        for proj in ("to_q", "to_k", "to_v"):
            names.add(getattr(mod, proj).weight, proj + ".weight")
        names.add(mod.to_out[0].weight, "to_out.weight")
        names.add(mod.to_out[0].bias, "to_out.bias")
        if spec["lora"]:
            mod.__dict__[attention.LORA_ATTR] = _Lora()
        hidden = torch.randn(spec["B"], spec["N"], C).to(_DT[spec["hidden_dtype"] or spec["dtype"]])
        hidden = names.add(hidden.as_subclass(FakeCuda) if spec["cuda"] else hidden, "hidden")
        ctx = None if spec["ctx"] == "none" else _context(spec, names, attention)
        log = []
        for op, stand_in in _stand_ins(spec, names, log, ops).items():
            patch(ops, op, stand_in)
        for _ in range(spec["runs"]):
            calls = []
            log.append(calls)
            try:
                if spec["entry"] == "and_out":
                    out, projected = attention._attention_and_out(mod, hidden, ctx), None
                else:
                    out, projected = attention._attention(mod, hidden, ctx, mod.to_out[0] if spec["out_linear"] else None)
                runs.append(dict(calls=calls, out=names.show(out), projected=projected))
            except attention.PwwHipError as e:
                runs.append(dict(calls=calls, error=str(e)))
        result = dict(runs=runs, warns=warns)
        if isinstance(ctx, dict):
            slots = ctx.get(attention.COEFF_SLOTS)
            if slots is not None:
                result["slots"] = dict(unsupported=slots.unsupported, cursor=slots.cursor, words=names.show(slots.dev[:slots.cursor].tolist()),
                                       sites=[(s["kind"], names.show(s["w"]), s["qk_shape"], str(s["dtype"])) for s in slots.sites])
            result["kv_cache"] = [(a is mod, names.show(kv)) for a, kv in ctx[attention.KV_CACHE].values()]
            result["orig_cache"] = {n: names.show(t) for n, t in ctx.get("_PWW_ORIG_CACHE", {}).items()}
            result["scratch"] = "_pww_fused_scratch" in mod.__dict__
        return result
    finally:
        for obj, attr, value in reversed(undo):
            setattr(obj, attr, value)


@pytest.mark.parametrize("name", sorted(CASES))
def test_attention_plan(name):
    from attn_plan_expected import EXPECTED
    assert record(name) == EXPECTED[name]


def test_the_table_covers_the_cases():
    from attn_plan_expected import EXPECTED
    assert sorted(EXPECTED) == sorted(CASES)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    print('"""What test_attention_plan_host.py recorded for every case of attn_plan_cases.py (`python tests/test_attention_plan_host.py`)."""')
    print("EXPECTED = {")
    for name in sorted(CASES):
        rec = record(name)
        print("    %r: {'runs': [" % name)
        for run in rec.pop("runs"):
            print("        {'calls': [")
            for call in run.pop("calls"):
                print("            %r," % (call,))
            print("        ], %s}," % repr(run)[1:-1])
        print("    ], %s}," % pprint.pformat(rec, width=10000, sort_dicts=False)[1:-1])
    print("}")
