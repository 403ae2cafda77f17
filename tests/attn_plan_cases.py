"""Case table of the attention plug's plan (pww_hip/attention.py:_attention): which ops launches a call makes, in which order and with which
arguments, for every kind of context, weight-function result, key count, row gate, hipGraph slot state, recorder state, switch, LoRA state and
map lookup. Plain Python, no GPU and no library: test_attention_plan_host.py runs every case with the ops launches replaced by recording
stand-ins and compares the record with attn_plan_expected.py (recorded from the code as it stood when the table was written).

A case is a name and the fields of DEFAULT it overrides:
  entry         "_attention" | "and_out" (attention._attention_and_out: FUSE_TO_OUT is read there)
  ctx           "none" (self-attention) | "tensor" | "dict"
  C, D          channels of the layer and head dim (heads = C // D); Cctx: channels of the context; N query tokens, M keys, B rows
  ctxB          rows of the context tensor (default B; 1 with LoRA: the K|V rows are expanded)
  dtype         of the module and the activations ("f16" | "f32"); ctx_dtype, hidden_dtype: of the context tensor / hidden_states (default: dtype)
  cuda          hidden_states says it is on the device (False: the plug refuses, the record holds the error text)
  bias_on       projections that carry a bias (a biased to_q / to_k keeps the fused projections away)
  f, sigma      weight function by name (FUNCTIONS) and SIGMA as a Python float or a 0-dim tensor
  gate          None | "rows" (_PWW_ROW_GATE alone) | "gated" (+ _PWW_GATED_ROWS) | "negative" (every row gated, _PWW_COND_ROWS present)
  slots         None | "fresh" | "unsupported": the CoeffSlots of the context
  rec           None | "on" | "muted": the AttentionRecorder of the context
  lora          a LoRA layer on the module
  map           "level" (CROSS_ATTENTION_WEIGHT_<N>) | "compact" | "compact_other" (a compact form beside the "orig" fallback: not of the map in use) | "orig" | "orig4" (batched) | "orig0"
  bias_cols     _PWW_BIAS_COLS
  out_linear    hand the layer's to_out[0] to _attention; out_supported: what ops.attention_out_supported answers
  qproj_ok      ops.qproj_parts answers 3 (else 0); scoped_lib: what ops.scoped_available answers
  runs          calls with the same context (2: the second finds the K|V cache)
  sw            module switches of pww_hip.attention set for the case (the others are set to their defaults)
"""
import math

import torch

DEFAULT = dict(entry="_attention", ctx="dict", C=64, D=32, Cctx=32, N=16, M=77, B=2, ctxB=None, dtype="f16", ctx_dtype=None, bias_on=(), f="zero",
               sigma="float", gate=None, slots=None, rec=None, lora=False, map="level", bias_cols=None, out_linear=False, out_supported=True,
               qproj_ok=True, scoped_lib=True, runs=1, sw={}, hidden_dtype=None, cuda=True)
SWITCHES = dict(FUSED_CROSS=False, FUSE_TO_OUT=False, SCOPED_STATS=True, QPROJ_STAT="1", _LAZY_W=True)


def _g(sigma):
    return torch.log(1 + sigma) if torch.is_tensor(sigma) else math.log(1 + sigma)


def _forced(w, sigma, qk):
    forced = float(torch.log(qk.max().abs() + 1).sum())     # the statistics now exist as a tensor
    return (0.3 + 0.0 * forced) * w * _g(sigma) * qk.max()


def _handmade(w, sigma, qk):
    from pww_hip.attention import ScaledW
    return ScaledW(w.w, torch.tensor(0.5), qk.max())        # a tensor coefficient beside a symbolic statistic


FUNCTIONS = {
    "zero": lambda w, sigma, qk: 0.0,
    "zero_tensor": lambda w, sigma, qk: torch.tensor(0.0),
    "bare_stat": lambda w, sigma, qk: qk.max(),
    "cw": lambda w, sigma, qk: 0.3 * w * _g(sigma),
    "max": lambda w, sigma, qk: 0.3 * w * _g(sigma) * qk.max(),
    "std": lambda w, sigma, qk: 0.3 * w * _g(sigma) * qk.std(),
    "mean": lambda w, sigma, qk: 0.3 * w * _g(sigma) * qk.mean(),
    "absmax": lambda w, sigma, qk: 0.3 * w * _g(sigma) * qk.abs().max(),
    "forced": _forced,
    "head": lambda w, sigma, qk: 0.3 * w * _g(sigma) * qk.amax(dim=(1, 2), keepdim=True),
    "row": lambda w, sigma, qk: 0.3 * w * _g(sigma) * qk.std(dim=-1, keepdim=True),
    "tensor": lambda w, sigma, qk: w + 1,
    "qk": lambda w, sigma, qk: qk,
    "handmade": _handmade,
}

QP0 = dict(sw=dict(QPROJ_STAT="0"))     # keep the to_q GEMM with the statistic away: C = 64 is on its yes-side


def _case(*parts, **kw):
    out = {}
    for p in parts:
        out.update(p)
    out.update(kw)
    return out


CASES = {
    # ---- context ----
    "self": dict(ctx="none"),
    "self_lora": dict(ctx="none", lora=True),
    "self_q_bias": dict(ctx="none", bias_on=("to_q",)),
    "self_q_bias_lora": dict(ctx="none", bias_on=("to_q",), lora=True),
    "self_f32": dict(ctx="none", dtype="f32"),
    "tensor": dict(ctx="tensor"),
    "tensor_lora": dict(ctx="tensor", lora=True, ctxB=1),
    "tensor_k_bias": dict(ctx="tensor", bias_on=("to_k",)),
    "tensor_k_bias_lora": dict(ctx="tensor", bias_on=("to_k",), lora=True),
    "tensor_f32_context": dict(ctx="tensor", ctx_dtype="f32"),
    "dict_zero": dict(),
    "dict_f32_hidden": dict(f="max", hidden_dtype="f32"),
    "dict_cpu_hidden": dict(f="max", cuda=False),
    "dict_second_call": dict(f="max", runs=2),
    "dict_second_call_lora": dict(f="max", runs=2, lora=True, ctxB=1),
    "dict_f32_context": dict(f="max", ctx_dtype="f32"),
    "dict_f32_module": dict(f="max", dtype="f32"),
    "dict_k_bias": dict(f="max", bias_on=("to_k",)),
    "dict_k_bias_lora": dict(f="max", bias_on=("to_k",), lora=True),
    "dict_q_bias": dict(f="max", bias_on=("to_q",)),
    # ---- what the weight function returns (to_q GEMM with the statistic: taken, then switched off) ----
    "f_zero_tensor": dict(f="zero_tensor"),
    "f_bare_stat": dict(f="bare_stat"),
    "f_cw": dict(f="cw"),
    "f_cw_tensor_sigma": dict(f="cw", sigma="tensor"),
    "f_max": dict(f="max"),
    "f_std": dict(f="std"),
    "f_mean": dict(f="mean"),
    "f_absmax": dict(f="absmax"),
    "f_max_qp0": _case(QP0, f="max"),
    "f_std_qp0": _case(QP0, f="std"),
    "f_mean_qp0": _case(QP0, f="mean"),
    "f_max_tensor_sigma": dict(f="max", sigma="tensor"),
    "f_forced": dict(f="forced"),
    "f_head": dict(f="head"),
    "f_row": dict(f="row"),
    "f_head_tensor_sigma": dict(f="head", sigma="tensor"),
    "f_tensor": dict(f="tensor"),
    "f_qk": dict(f="qk"),
    "f_handmade": dict(f="handmade"),
    "f_max_qproj_unsupported": dict(f="max", qproj_ok=False),
    # ---- key counts: the edges of FUSED_MAX_KEYS and LONG_MAX_KEYS ----
    **{"keys_max_%d" % M: dict(f="max", M=M) for M in (77, 128, 129, 154, 256, 257)},
    **{"keys_max_qp0_%d" % M: _case(QP0, f="max", M=M) for M in (128, 129)},
    **{"keys_cw_slots_%d" % M: dict(f="cw", slots="fresh", M=M) for M in (77, 128, 129, 154, 256, 257)},
    **{"keys_forced_%d" % M: dict(f="forced", M=M) for M in (128, 154, 257)},
    **{"keys_head_%d" % M: dict(f="head", M=M) for M in (128, 129)},
    **{"keys_row_%d" % M: dict(f="row", M=M) for M in (128, 129)},
    "keys_zero_257": dict(M=257),
    "keys_tensor_154": dict(f="tensor", M=154),
    # ---- row gate ----
    **{"gate_%s_%s" % (g, f): _case(QP0, f=f, gate=g) for g in ("rows", "gated", "negative") for f in ("max", "head", "row", "zero", "tensor")},
    **{"gate_%s_cw_tensor_sigma" % g: dict(f="cw", sigma="tensor", gate=g) for g in ("gated", "negative")},
    **{"gate_%s_cw" % g: dict(f="cw", gate=g) for g in ("gated", "negative")},
    "gate_gated_max_qproj": dict(f="max", gate="gated"),
    "gate_gated_max_154": dict(f="max", gate="gated", M=154),
    # ---- hipGraph slots ----
    **{"slots_%s_%s" % (s, f): dict(f=f, slots=s) for s in ("fresh", "unsupported")
       for f in ("zero", "zero_tensor", "bare_stat", "cw", "max", "head", "row", "tensor", "qk", "forced")},
    **{"slots_%s_cw_tensor_sigma" % s: dict(f="cw", sigma="tensor", slots=s) for s in ("fresh", "unsupported")},
    "slots_fresh_max_qp0": _case(QP0, f="max", slots="fresh"),
    "slots_fresh_max_154": dict(f="max", slots="fresh", M=154),
    "slots_fresh_max_second_call": dict(f="max", slots="fresh", runs=2),
    "slots_fresh_tensor_ctx": dict(ctx="tensor", slots="fresh"),
    # ---- recorder ----
    "rec_zero": dict(rec="on"),
    "rec_plain": dict(rec="on", f="cw", sigma="tensor"),
    "rec_plain_python_coeff": dict(rec="on", f="cw"),
    "rec_tensor": dict(rec="on", f="tensor"),
    "rec_stat": dict(rec="on", f="forced"),
    "rec_parts_qproj": dict(rec="on", f="max"),
    "rec_parts": _case(QP0, rec="on", f="max"),
    "rec_parts_slots": _case(QP0, rec="on", f="max", slots="fresh"),
    "rec_parts_none": dict(rec="on", f="cw", slots="fresh"),
    "rec_long": dict(rec="on", f="max", M=154),
    "rec_long_none": dict(rec="on", f="cw", slots="fresh", M=154),
    "rec_long_256": dict(rec="on", f="std", M=256),
    "rec_fused": dict(rec="on", f="max", sw=dict(FUSED_CROSS=True, QPROJ_STAT="0")),
    "rec_fused_qproj": dict(rec="on", f="max", sw=dict(FUSED_CROSS=True)),
    "rec_refused_257": dict(rec="on", f="max", M=257),
    "rec_refused_257_none": dict(rec="on", f="cw", slots="fresh", M=257),
    "rec_head": dict(rec="on", f="head"),
    "rec_to_out": dict(rec="on", f="max", out_linear=True),
    "rec_muted_parts": _case(QP0, rec="muted", f="max"),
    "rec_muted_long": dict(rec="muted", f="max", M=154),
    "rec_muted_zero": dict(rec="muted"),
    "rec_gated_parts": _case(QP0, rec="on", f="max", gate="gated"),
    "rec_negative_parts": _case(QP0, rec="on", f="max", gate="negative"),
    "rec_tensor_ctx": dict(ctx="tensor", rec="on"),
    # ---- switches ----
    "fused_cross": dict(f="max", sw=dict(FUSED_CROSS=True)),
    "fused_cross_qp0": dict(f="max", sw=dict(FUSED_CROSS=True, QPROJ_STAT="0")),
    "fused_cross_second_call": dict(f="max", sw=dict(FUSED_CROSS=True, QPROJ_STAT="0"), runs=2),
    "fused_cross_154": dict(f="max", M=154, sw=dict(FUSED_CROSS=True)),
    "fused_cross_forced": dict(f="forced", sw=dict(FUSED_CROSS=True)),
    "fused_cross_cw_slots": dict(f="cw", slots="fresh", sw=dict(FUSED_CROSS=True)),
    "scoped_off_head": dict(f="head", sw=dict(SCOPED_STATS=False)),
    "scoped_off_row": dict(f="row", sw=dict(SCOPED_STATS=False)),
    "scoped_no_library": dict(f="head", scoped_lib=False),
    "scoped_out_linear": dict(f="head", out_linear=True),
    **{"qproj_%s_c320" % q: dict(f="max", C=320, D=40, sw=dict(QPROJ_STAT=q)) for q in ("0", "1", "all")},
    **{"qproj_%s_c1280" % q: dict(f="max", C=1280, D=160, sw=dict(QPROJ_STAT=q)) for q in ("0", "1", "all")},
    "qproj_all_cw_slots": dict(f="cw", slots="fresh", sw=dict(QPROJ_STAT="all")),
    "to_out_yes": dict(entry="and_out", f="max", sw=dict(FUSE_TO_OUT=True)),
    "to_out_no": dict(entry="and_out", f="max", out_supported=False, sw=dict(FUSE_TO_OUT=True)),
    "to_out_switch_off": dict(entry="and_out", f="max"),
    "to_out_direct_yes": dict(f="max", out_linear=True),
    "to_out_direct_no": dict(f="max", out_linear=True, out_supported=False),
    "to_out_direct_154": dict(f="max", out_linear=True, M=154),
    "to_out_direct_forced": dict(f="forced", out_linear=True),
    "to_out_direct_cw_slots": dict(f="cw", slots="fresh", out_linear=True, gate="gated", bias_cols=40),
    "to_out_direct_fused_cross": dict(f="max", out_linear=True, sw=dict(FUSED_CROSS=True, QPROJ_STAT="0")),
    "to_out_direct_plain": dict(f="cw", sigma="tensor", out_linear=True),
    "to_out_direct_zero": dict(out_linear=True),
    "lazy_w_off_max": dict(f="max", sw=dict(_LAZY_W=False)),
    "lazy_w_off_cw": dict(f="cw", sw=dict(_LAZY_W=False)),
    "lazy_w_off_zero_slots": dict(slots="fresh", sw=dict(_LAZY_W=False)),
    # ---- LoRA ----
    "lora_max_qproj_all": dict(f="max", lora=True, ctxB=1, sw=dict(QPROJ_STAT="all")),
    "lora_to_out": dict(entry="and_out", f="max", lora=True, ctxB=1, sw=dict(FUSE_TO_OUT=True)),
    "lora_and_out_self": dict(entry="and_out", ctx="none", lora=True),
    "lora_head": dict(f="head", lora=True, ctxB=1),
    "lora_zero_full_context": dict(lora=True),
    # ---- map lookup ----
    "map_compact": _case(QP0, f="max", map="compact"),
    "map_compact_qproj": dict(f="max", map="compact"),
    "map_compact_other": _case(QP0, f="max", map="compact_other"),
    "map_compact_cw": dict(f="cw", map="compact"),
    "map_bias_cols": _case(QP0, f="max", bias_cols=40),
    "map_bias_cols_gated_154": dict(f="max", bias_cols=40, gate="gated", M=154),
    "map_orig": _case(QP0, f="max", map="orig"),
    "map_orig_second_call": _case(QP0, f="max", map="orig", runs=2),
    "map_orig4": _case(QP0, f="max", map="orig4"),
    "map_orig_slots": dict(f="cw", map="orig", slots="fresh"),
    "map_orig0": dict(f="max", map="orig0"),
    "map_orig0_slots": dict(f="max", map="orig0", slots="fresh"),
}
