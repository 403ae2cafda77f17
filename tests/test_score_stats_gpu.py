"""Every producer of the score statistic (max, min, sum, sum of squares of Q K^T) on the cases of tests/stat_cases.py, in fp16 and bf16, against
an fp64 reference on the same rounded inputs -- independent of the kernels' family (torch matmul), computed on the GPU.

Per case of qk_parts, long_qk_parts, scope_head_parts and qproj_stat, over the variants neg, pos, probe_neg, probe_pos and view:
  1. the partials of STAT_ALL folded with ops.fold_parts: max and min EQUAL the reference (the dyadic scores are exact in fp32), sum and sum
     of squares within 1e-6 cnt max|s| and 1e-6 of the reference (the bars of the existing tests); qproj_stat: the returned Q equals the fp64
     product cast to the storage type. scope_head_parts takes no STAT_ALL: the fields of its MAX, MIN and STD launches stand in;
  2. (every variant) each of STAT_MAX / MIN / ABSMAX / MEAN / STD alone writes the bits of STAT_ALL in the fields it owns and the neutral element
     (-inf, +inf, 0, 0) in the others;
  3. a second call returns the same bits; view: no NaN, bit-identical to the same call on contiguous copies;
  4. (every variant) with the last image of a batch gated out, the launch into a sentinel-filled buffer leaves that image's rows untouched and writes the
     other images' bits;
  5. shifted (non-zero mean, not dyadic): the sums within the forward rounding bound (D + L + 2) u sum(|q| . |k|) and (2 D + L + 4) u sum(s^2),
     u = 2^-24, L = stat_cases.lane_chain; the resulting mean / unbiased standard deviation errors are printed (recorded, not asserted).
qk_stats (no partials, no gate, no field selection): 1, 3 and 5 on its [B, 4] result, and its 2 / 4-wave rule tied to the library's.
Row scope: ops.attention_scoped(scope=SCOPE_ROW) for the five kinds on one-signed scores against stat_cases.row_oracle (compared here with
the fp64 oracle of test_scoped_stats_gpu.py) under its bar. Fold: synthetic fp64 partials through stats_out= of ops.attention (lean launch,
general launch: the kernel that ran is read from the debug timeline) and of attention_scoped."""
import ctypes
import math

import pytest
import torch

import stat_cases as sc
from gpu_util import TOL, last_attn_route

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
KIND_FIELDS = {"MAX": [0], "MIN": [1], "ABSMAX": [0, 1], "MEAN": [2], "STD": [2, 3]}
NEUTRAL = (-math.inf, math.inf, 0.0, 0.0)


@pytest.fixture(scope="module")
def side_libs(gpu_device):
    """libpww_hip_long.so and libpww_hip_scope.so, built in-tree when missing (the module builds / locates them itself)"""
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_long()
    pww_build.build_scope()
    libs = {"main": _lib.load(), "long": _lib.load_long(), "scope": _lib.load_scope()}
    assert all(lib is not None for lib in libs.values())
    return libs


def _produce(case, inp, kind, gate=None):
    """The wrapper of the case's kernel -> partials [B, P, 4] ([B, H, P, 4] for scope_head_parts; qproj_stat: (partials, q))"""
    from pww_hip import ops
    k = getattr(ops, "STAT_" + kind)
    if case.kernel == "qk_parts":
        return ops.qk_parts(inp["q"], inp["k"], case.H, k, gate=gate)
    if case.kernel == "long_qk_parts":
        return ops.long_qk_parts(inp["q"], inp["k"], case.H, k, gate=gate)
    if case.kernel == "scope_head_parts":
        return ops.scope_head_parts(inp["q"], inp["k"], case.H, k, gate=gate)
    q, parts = ops.qproj_stat(inp["x"], inp["w"], inp["k"], case.H, k, gate=gate)
    return parts, q


def _launch_into(libs, case, inp, kind, gate, parts):
    """The C entry point itself into a caller-filled partials buffer (the wrappers allocate their own)"""
    from pww_hip import _lib, ops
    k, nbytes = int(getattr(ops, "STAT_" + kind)), parts.numel() * 8
    if case.kernel == "qproj_stat":
        q = torch.empty(inp["q"].shape, dtype=inp["q"].dtype, device=inp["q"].device)
        d = ops._qproj_desc(inp["x"], inp["w"], inp["k"], case.H)
        d.q_stride[:] = [q.stride(0), q.stride(1)]
        _lib.check(libs["main"].pww_qproj_stat(ops._ptr(inp["x"]), ops._ptr(inp["w"]), ops._ptr(q), ops._ptr(inp["k"]), ops._ptr(gate), ctypes.byref(d), k,
                                               ops._ptr(parts), nbytes, ops._stream()), "pww_qproj_stat")
        return
    d = ops._desc(inp["q"], inp["k"], None, None, case.H, 1.0)
    args = (ops._ptr(inp["q"]), ops._ptr(inp["k"]), ops._ptr(gate), ctypes.byref(d), k)
    if case.kernel == "qk_parts":
        _lib.check(libs["main"].pww_qk_parts(*args, 0, ops._ptr(parts), nbytes, ops._stream()), "pww_qk_parts")
    elif case.kernel == "long_qk_parts":
        _lib.check(libs["long"].pww_long_qk_parts(*args, 0, ops._ptr(parts), nbytes, ops._stream()), "pww_long_qk_parts", libs["long"])
    else:
        _lib.check(libs["scope"].pww_scope_head_parts(*args, ops._ptr(parts), nbytes, ops._stream()), "pww_scope_head_parts", libs["scope"])


def _all_fields(case, inp):
    """Partials with all four fields: STAT_ALL, or for scope_head_parts (one statistic per launch) the fields of MAX, MIN and STD"""
    if case.kernel != "scope_head_parts":
        out = _produce(case, inp, "ALL")
        return out if case.kernel == "qproj_stat" else (out, None)
    mx, mn, sd = (_produce(case, inp, kd) for kd in ("MAX", "MIN", "STD"))
    return torch.stack([mx[..., 0], mn[..., 1], sd[..., 2], sd[..., 3]], dim=-1), None


def _folded(parts):
    from pww_hip import ops
    if parts.dim() == 3:
        return ops.fold_parts(parts)
    B, H, P, _ = parts.shape
    return ops.fold_parts(parts.reshape(B * H, P, 4)).reshape(B, H, 4)


def _check_fields(got, s, variant, case, tag, failures, q=None, k=None):
    """got [.., 4] against the fp64 fields of the scores s: extremes by equality (dyadic variants), sums under sc.sum_bars. Prints the
    observed figures and returns them (sum error / bar, sum-of-squares error / bar)."""
    scope = "head" if got.dim() == 3 else "image"
    ref = sc.fields(s, scope)
    bar_sum, bar_sq = sc.sum_bars(s, variant, case, q, k)
    e_sum = ((got[..., 2] - ref[..., 2]).abs() / bar_sum).max().item()
    e_sq = ((got[..., 3] - ref[..., 3]).abs() / bar_sq).max().item()
    if variant != "shifted":
        for f, name in ((0, "max"), (1, "min")):
            if not torch.equal(got[..., f], ref[..., f]):
                failures.append("%s: %s %s, the reference has %s" % (tag, name, got[..., f].flatten().tolist()[:8], ref[..., f].flatten().tolist()[:8]))
    if not e_sum <= 1.0:
        failures.append("%s: |sum - ref| = %.3e of its bar" % (tag, e_sum))
    if not e_sq <= 1.0:
        failures.append("%s: |sumsq - ref| = %.3e of its bar" % (tag, e_sq))
    cnt = s.numel() // ref[..., 0].numel()
    (m, sd), (m0, sd0) = sc.mean_std(got, cnt), sc.mean_std(ref, cnt)
    e_mean, e_std = ((m - m0).abs() / sd0.clamp_min(1e-300)).max().item(), ((sd - sd0).abs() / sd0.clamp_min(1e-300)).max().item()
    print("STATS %s: sum %.3e of its bar, sumsq %.3e of its bar; mean off by %.3e std, std off by %.3e std" % (tag, e_sum, e_sq, e_mean, e_std))
    return e_sum, e_sq


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", [c for c in sc.CASES if c.kernel == "qk_stats"], ids=lambda c: c.name)
def test_qk_stats(gpu_device, case, dtype):
    from pww_hip import ops
    failures = []
    # the 2 / 4-wave form: dispatch_reduce asks the rule the general attention launch asks (attn_wide_groups_rule), and that launch reports
    # its row groups -- a self-attention call of the case's (B, H, N, D) takes 4 or 8 of them exactly where qk_reduce_kernel takes 4 waves
    inp = sc.to_device(sc.build(case, dtype, "neg"), gpu_device)
    ops.attention(inp["q"], inp["k"], inp["k"], case.H, case.D ** -0.5)
    assert (last_attn_route()[3] >= 4) == (case.form[0] == 4), "%s: the wide-groups rule of the library is not the model's" % case.name
    for variant in sc.VARIANTS + ("shifted",):
        inp = sc.to_device(sc.build(case, dtype, variant), gpu_device)
        call = sc.as_views(inp) if variant == "view" else inp
        got = ops.qk_stats(call["q"], call["k"], case.H)
        assert torch.equal(got, ops.qk_stats(call["q"], call["k"], case.H)), "%s %s: a second call differs" % (case.name, variant)
        if variant == "view":
            assert not call["q"].is_contiguous() and not call["k"].is_contiguous() and ops._rows_ok(call["q"]) and ops._rows_ok(call["k"])
            assert not torch.isnan(got).any()
            assert torch.equal(got, ops.qk_stats(inp["q"], inp["k"], case.H)), "%s: strided views and contiguous copies differ" % case.name
        s = sc.scores(inp["q"], inp["k"], case.H)
        _check_fields(got, s, variant, case, "%s %s %s" % (case.name, str(dtype)[6:], variant), failures, inp["q"], inp["k"])
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", [c for c in sc.CASES if c.kernel != "qk_stats"], ids=lambda c: c.name)
def test_partials(gpu_device, side_libs, case, dtype):
    from pww_hip import ops
    failures = []
    tagp = "%s %s" % (case.name, str(dtype)[6:])
    for variant in sc.VARIANTS + ("shifted",):
        tag = "%s %s" % (tagp, variant)
        inp = sc.to_device(sc.build(case, dtype, variant), gpu_device)
        call = sc.as_views(inp) if variant == "view" else inp
        parts, q = _all_fields(case, call)
        assert parts.shape[-2] == sc.case_parts(case), "%s: %d partials, the model has %d" % (tag, parts.shape[-2], sc.case_parts(case))
        again, q2 = _all_fields(case, call)
        assert torch.equal(parts, again) and (q is None or torch.equal(q, q2)), "%s: a second call differs" % tag
        assert not torch.isnan(parts).any()
        if variant == "view":
            names = ("x", "k") if case.kernel == "qproj_stat" else ("q", "k")
            assert all(not call[n].is_contiguous() and ops._rows_ok(call[n]) for n in names)
            plain, qc = _all_fields(case, inp)
            assert torch.equal(parts, plain) and (q is None or torch.equal(q, qc)), "%s: strided views and contiguous copies differ" % tag
        if q is not None:
            if variant == "shifted":
                inp = dict(inp, q=q)             # (the statistics are those of the rounded Q the kernel returns)
            elif not torch.equal(q, inp["q"]):
                failures.append("%s: the returned Q is not the fp64 product cast to the storage type" % tag)
        s = sc.scores(inp["q"], inp["k"], case.H)
        _check_fields(_folded(parts), s, variant, case, tag, failures, inp["q"], inp["k"])
        if variant == "shifted":
            continue
        # ---- field selection: the bits of STAT_ALL in the fields a statistic owns, the neutral element in the others
        for kind, owned in KIND_FIELDS.items():
            one = _produce(case, call, kind)
            one = one[0] if case.kernel == "qproj_stat" else one
            for f in range(4):
                want = parts[..., f] if f in owned else torch.full_like(parts[..., f], NEUTRAL[f])
                if not torch.equal(one[..., f], want):
                    failures.append("%s: STAT_%s writes field %d differently from %s" % (tag, kind, f, "STAT_ALL" if f in owned else "the neutral element"))
        # ---- gating: the last image gated out (the only one of a batch of 1), its rows of a sentinel-filled buffer stay as they are
        gate = torch.ones(case.B, dtype=torch.float32, device=gpu_device)
        gate[-1] = 0.0
        for kind in ("MAX", "STD") if case.kernel == "scope_head_parts" else ("ALL",):
            buf = torch.full_like(parts, SENTINEL)
            _launch_into(side_libs, case, call, kind, gate, buf)
            assert bool((buf[-1] == SENTINEL).all()), "%s: the gated-out image's partials were written" % tag
            owned = KIND_FIELDS.get(kind, [0, 1, 2, 3])
            assert torch.equal(buf[:-1][..., owned], parts[:-1][..., owned]), "%s: gating an image out changes the others" % tag
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", sc.ROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_scope_on_one_signed_scores(gpu_device, side_libs, shape, dtype):
    import test_scoped_stats_gpu as tsg
    from pww_hip import ops
    B, H, N, M, D = shape
    failures = []
    for variant in ("neg", "pos"):
        inp = sc.to_device(sc.row_inputs(shape, dtype, variant), gpu_device)
        for kind in KIND_FIELDS:
            k = getattr(ops, "STAT_" + kind)
            out = ops.attention_scoped(inp["q"], inp["k"], inp["v"], H, inp["scale"], inp["w"], k, ops.SCOPE_ROW, inp["scalar"])
            assert torch.equal(out, ops.attention_scoped(inp["q"], inp["k"], inp["v"], H, inp["scale"], inp["w"], k, ops.SCOPE_ROW, inp["scalar"]))
            ref = sc.row_oracle(inp, kind)
            if variant == "neg":         # (the same oracle as the existing row-scope tests use)
                theirs, _ = tsg._oracle(inp["q"], inp["k"], inp["v"], H, inp["scale"], inp["w"], k, "row", inp["scalar"])
                assert (ref - theirs).abs().max().item() <= 1e-12 * ref.abs().max().item()
            err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
            print("ROW %s %s %s %s: max err / max|O| = %.3e (bar %.1e)" % (shape, variant, kind, str(dtype)[6:], err, TOL[dtype]))
            if torch.isnan(out).any() or not err <= TOL[dtype]:
                failures.append("%s %s: %.3e" % (variant, kind, err))
    assert not failures, "; ".join(failures)


def _check_fold(stats_out, parts, tag, owned=(0, 1, 2, 3)):
    """stats_out against the torch fold: extremes equal, sums to 1e-12 relative (fp64 sums in a fixed order); fields the launch's statistic
    does not own hold the neutral element"""
    want = sc.fold(parts)
    for f in (0, 1):
        expect = want[..., f] if f in owned else torch.full_like(want[..., f], NEUTRAL[f])
        assert torch.equal(stats_out[..., f], expect), "%s: field %d is %s, torch folds %s" % (tag, f, stats_out[..., f].tolist(), expect.tolist())
    for f in (2, 3):
        if f in owned:
            rel = ((stats_out[..., f] - want[..., f]).abs() / want[..., f].abs()).max().item()
            print("FOLD %s: field %d off by %.3e relative" % (tag, f, rel))
            assert rel <= 1e-12, "%s: field %d off by %.3e relative" % (tag, f, rel)
        else:
            assert bool((stats_out[..., f] == 0).all()), "%s: field %d is not neutral" % (tag, f)


def _cross_launch(fn):
    """fn() under pww_debug_timeline: its result and which cross-attention kernel ran, read from the phase stamps of workgroup 0 -- the
    general kernel stamps its exit in slot 5, the one-block-per-workgroup kernel of pww_cross_lean.hip ends with slot 4 and leaves 5 alone"""
    from pww_hip import _lib
    lib = _lib.load()
    stamps = torch.zeros(64, 8, dtype=torch.int64, device="cuda")
    lib.pww_debug_timeline(ctypes.c_void_p(stamps.data_ptr()), stamps.numel() * 8)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.pww_debug_timeline(None, 0)
    first = stamps[0].tolist()
    return out, "general" if first[5] else "lean" if first[4] else "none"


@pytest.mark.parametrize("launch", ["lean", "general"])
@pytest.mark.parametrize("P", sc.FOLD_COUNTS)
def test_fold_of_caller_made_partials(gpu_device, launch, P):
    """stats_out of ops.attention(parts=...) on synthetic partials: M = 64 takes the lean launch, M = 33 the general launch with external partials"""
    from pww_hip import ops
    B, H, N, M, D = sc.FOLD_SHAPES[launch]
    g = torch.Generator().manual_seed(sc.SEED + P)
    q, k, v = (torch.randn(B, n, H * D, generator=g).to(gpu_device, torch.float16) for n in (N, M, M))
    w = torch.rand(N, M, generator=g).to(gpu_device)
    parts = sc.synthetic_parts((B,), P, P).to(gpu_device)
    for kind in ("MAX", "STD"):
        stats_out = torch.full((B, 4), SENTINEL, dtype=torch.float64, device=gpu_device)
        out, took = _cross_launch(lambda: ops.attention(q, k, v, H, D ** -0.5, bias=w, stat=(None, getattr(ops, "STAT_" + kind), 0.125), parts=parts,
                                                        stats_out=stats_out))
        assert took == launch, "the %s launch was meant, the %s kernel ran" % (launch, took)
        assert not torch.isnan(out).any()
        _check_fold(stats_out, parts, "%s P = %d %s" % (launch, P, kind))


@pytest.mark.parametrize("P", sc.SCOPE_FOLD_COUNTS)
def test_fold_of_caller_made_partials_head_scope(gpu_device, side_libs, P):
    from pww_hip import ops
    B, H, M, D = 1, 2, 5, 8
    N = sc.scope_fold_rows(P)
    g = torch.Generator().manual_seed(sc.SEED + P)
    q, k, v = (torch.randn(B, n, H * D, generator=g).to(gpu_device, torch.bfloat16) for n in (N, M, M))
    w = torch.rand(N, M, generator=g).to(gpu_device)
    parts = sc.synthetic_parts((B, H), P, 1000 + P).to(gpu_device)
    for kind in ("ABSMAX", "STD"):          # (this launch folds the fields of its statistic only)
        stats_out = torch.full((B, H, 4), SENTINEL, dtype=torch.float64, device=gpu_device)
        out = ops.attention_scoped(q, k, v, H, D ** -0.5, w, getattr(ops, "STAT_" + kind), ops.SCOPE_HEAD, 0.125, parts=parts, stats_out=stats_out)
        assert not torch.isnan(out).any()
        _check_fold(stats_out, parts, "head scope P = %d %s" % (P, kind), KIND_FIELDS[kind])
