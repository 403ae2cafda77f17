"""The case tables, inputs and dispatch models of tests/stat_cases.py, checked without a GPU: the models agree with the libraries' own host-only
counters, every case takes the form it is in the table for, the tables reach every form, and -- on the fp64 reference alone -- every field
the GPU test (test_score_stats_gpu.py) asserts changes under each emulated fault (stat_cases.emulate): a kernel with that fault cannot pass."""
import ctypes
import math

import pytest
import torch

import stat_cases as sc
from gpu_util import TOL

# every form the host code of the producers can launch, written out (not derived from the table)
EXPECTED_FORMS = {
    # D > 96 is wide whatever the row count
    "qk_stats": {(2, 3), (2, 4), (2, 5), (2, 6), (4, 3), (4, 4), (4, 5), (4, 6), (4, 8), (4, 10)},
    "qk_parts": {(f, ks) for f in ("fine", "coarse") for ks in sc.KS_CLASSES},
    "long_qk_parts": {("fine", 1), ("coarse", 1), ("coarse", 2)},
    "scope_head_parts": {(1, 3), (1, 4), (1, 10)},             # (more than one row block per wave needs N > 32768)
}
QPROJ_TILE_FORMS = {(5, 4, 1, 1, 4), (5, 4, 1, 1, 2), (5, 2, 1, 2, 3), (5, 1, 1, 4, 2), (10, 2, 2, 1, 3), (10, 1, 2, 2, 2)}
QPROJ_UNIT_FORMS = {(1, 0), (2, 0), (3, 0), (4, 0), (3, 3), (3, 4), (3, 5), (3, 10)}
KEY_COUNTS = {"qk_stats": {1, 63, 64, 65, 129, 200}, "qk_parts": {1, 32, 33, 64, 77, 96, 97, 128}, "long_qk_parts": {129, 160, 161, 231, 256},
              "scope_head_parts": {5, 32, 77, 97, 128}, "qproj_stat": {5, 32, 33, 64, 77, 96, 97, 128}}
ROW_COUNTS = {"qk_stats": {1, 63, 65, 129, 1000}, "qk_parts": {1, 31, 33, 70, 1100}, "long_qk_parts": {33, 70, 4200},
              "scope_head_parts": {1, 33, 128, 129, 1056}, "qproj_stat": {70, 2900, 8100}}
HEAD_DIMS = {"qk_stats": {8, 40, 64, 80, 96, 128, 160}, "qk_parts": {8, 40, 64, 80, 96, 128, 160}, "scope_head_parts": {8, 40, 64, 160}}


@pytest.fixture(scope="module")
def libs(built_lib):
    """libpww_hip.so and the long / scope libraries, built in-tree when missing (the module locates them itself)"""
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_long()
    pww_build.build_scope()
    return {"main": _lib.load(), "long": _lib.load_long(), "scope": _lib.load_scope()}


def _attn_desc(B, H, N, M, D):
    from pww_hip._lib import AttnDesc
    d = AttnDesc()
    d.dtype, d.B, d.H, d.N, d.M, d.D = 0, B, H, N, M, D
    C = H * D
    d.q_stride[:] = [N * C, D, C]
    d.k_stride[:] = [M * C, D, C]
    return d


def _qproj_desc(B, N, Cin, H, D, M):
    from pww_hip._lib import QprojDesc
    d = QprojDesc()
    d.dtype, d.B, d.N, d.Cin, d.H, d.D, d.M = 0, B, N, Cin, H, D, M
    d.x_stride[:] = [N * Cin, Cin]
    d.q_stride[:] = [N * H * D, H * D]
    d.k_stride[:] = [M * H * D, H * D]
    return d


def _library_count(libs, kernel, B, H, N, M, D, Cin=0):
    if kernel == "qproj_stat":
        return libs["main"].pww_qproj_parts(ctypes.byref(_qproj_desc(B, N, Cin, H, D, M)))
    fn = {"qk_parts": libs["main"].pww_qk_parts_count, "long_qk_parts": libs["long"].pww_long_qk_parts_count,
          "scope_head_parts": libs["scope"].pww_scope_head_parts_count}[kernel]
    return fn(ctypes.byref(_attn_desc(B, H, N, M, D)))


def test_models_match_the_libraries_counters(libs):
    """The Python models of the fine / coarse rules and of qproj_plan give the partial counts of pww_qk_parts_count, pww_long_qk_parts_count,
    pww_scope_head_parts_count and pww_qproj_parts over a grid that crosses every threshold."""
    rows = (1, 31, 32, 33, 70, 128, 129, 1000, 1056, 1100, 4096, 4097, 4200, 32768, 32769, 40000)
    for H in (1, 2, 8, 16, 20):
        for N in rows:
            for D in (8, 40, 64, 160):
                for M in (1, 32, 33, 77, 128):
                    assert _library_count(libs, "qk_parts", 2, H, N, M, D) == sc.model_qk_parts(2, H, N, M, D)[1], (H, N, M, D)
                    assert _library_count(libs, "scope_head_parts", 2, H, N, M, D) == sc.model_scope_head_parts(2, H, N, M, D)[1], (H, N, M, D)
                for M in (129, 160, 231, 256):
                    assert _library_count(libs, "long_qk_parts", 2, H, N, M, D) == sc.model_long_qk_parts(2, H, N, M, D)[1], (H, N, M, D)
    checked = 0
    for B in (1, 2):
        for N in (1, 64, 70, 256, 2900, 4096, 8100):
            for Cin in (64, 128, 192, 256, 320):
                for H, D in ((32, 40), (8, 40), (5, 64), (20, 64), (2, 160), (5, 32), (20, 8), (4, 80), (7, 40), (3, 48)):
                    for M in (5, 64, 77, 97, 128):
                        m = sc.model_qproj(B, N, Cin, H, D, M)
                        got = _library_count(libs, "qproj_stat", B, H, N, M, D, Cin)
                        assert got == (m[2] if m else 0), (B, N, Cin, H, D, M, got, m)
                        checked += m is not None
    assert checked > 1000


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_case_takes_its_form(libs, case):
    """The form in the table is the one the dispatch model gives, the model's partial count is the library's, and for qproj_stat the tile
    shape and ring read back from the library's count alone are the case's."""
    assert sc.case_form(case) == case.form
    assert case.D % 8 == 0 and case.D <= 160 and (case.H * case.D) % 8 == 0
    if case.kernel == "qk_stats":
        return
    count = _library_count(libs, case.kernel, case.B, case.H, case.N, case.M, case.D, case.Cin)
    assert count == sc.case_parts(case) > 0
    if case.kernel == "qproj_stat":
        assert sc.qproj_tile_from_count(case.B, case.N, case.Cin, case.H, case.D, case.M, count) == case.form[0]
        assert sc.qproj_lds(case.form[0][:4], case.M) <= sc.QPROJ_LDS_LIMIT


def test_tables_cover_every_form():
    by_kernel = {kn: [c for c in sc.CASES if c.kernel == kn] for kn in sc.KERNELS}
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)
    for kn, want in EXPECTED_FORMS.items():
        forms = {c.form[:2] for c in by_kernel[kn]}
        assert forms == want, kn
    assert {c.form[2] for c in by_kernel["long_qk_parts"]} >= {3, 4, 5, 6, 8, 10}
    assert {c.form[0] for c in by_kernel["qproj_stat"]} == QPROJ_TILE_FORMS
    assert {c.form[1] for c in by_kernel["qproj_stat"]} == QPROJ_UNIT_FORMS
    for kn, cases in by_kernel.items():
        assert {c.M for c in cases} == KEY_COUNTS[kn], kn
        assert {c.N for c in cases} == ROW_COUNTS[kn], kn
        if kn in HEAD_DIMS:
            assert {c.D for c in cases} == HEAD_DIMS[kn], kn
        # padding in rows and in keys within every form; every probe position somewhere; a batch to gate an image out of; K shared once
        for form in {c.form for c in cases}:
            assert any(c.N % 32 for c in cases if c.form == form), (kn, form)
        assert any(c.M % 32 for c in cases) and any(c.M % 32 == 0 for c in cases), kn
        assert all(sc.probes(c)[0][0] == (c.N - 1, c.M - 1) for c in cases), kn
        # every edge position carries a planted extreme (near or far probe) somewhere
        assert {sc.probe_positions(c.N, c.M).index(pr) for c in cases if not c.shared and c.N > 32 and c.M > 32 for pair in sc.probes(c) for pr in pair if pr} == {0, 1, 2, 3}, kn
        assert any(c.B >= 2 for c in cases) and any(c.shared for c in cases), kn
    qp = by_kernel["qproj_stat"]
    # each tile shape once with the 77-token prompt, except <10, 1, 2, 2>, whose LDS holds at most two key blocks beside its staging planes
    for tile in sc.QPROJ_TILES:
        assert any(c.M == 77 for c in qp if c.form[0][:4] == tile) == (tile != (10, 1, 2, 2)), tile
    assert all(sc.qproj_lds((10, 1, 2, 2), M) > sc.QPROJ_LDS_LIMIT for M in (65, 77, 128)) and sc.qproj_lds((10, 1, 2, 2), 64) <= sc.QPROJ_LDS_LIMIT
    # a ring longer than the contraction (chunks per contraction wave < NSETS), and heads of 160 channels only ever in 160-channel tiles
    assert any(c.Cin // (64 * c.form[0][3]) < c.form[0][4] for c in qp) and any(c.Cin // (64 * c.form[0][3]) > c.form[0][4] for c in qp)
    assert all(sc.model_qproj(B, N, Cin, H, 160, 77)[0][0] == 5 for B in (1, 2) for N in (1, 64, 70, 129, 300, 5000) for Cin in (64, 128, 256) for H in (2, 4, 8))
    # the coarse form of qk_parts with a row-block count that is no multiple of 4: the last workgroup has a wave without rows
    assert all(sc.cdiv(c.N, 32) % 4 for c in by_kernel["qk_parts"] if c.form[0] == "coarse")
    assert any(sc.cdiv(c.N, 32) % (4 * c.form[1]) for c in by_kernel["long_qk_parts"] if c.form[:2] == ("coarse", 2))


def _check_exact(s):
    """dyadic inputs: scores multiples of 1/32 below 256 (13 bits: exact in fp32 in any order)"""
    assert bool(((s * 32) == (s * 32).round()).all()) and s.abs().max().item() < 256


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_every_asserted_field_discriminates(case):
    """On the fp64 reference alone: for each variant the fields the GPU test asserts differ from each emulated fault -- the extremes in
    value, the sums by more than the bar they are checked with (shifted: the forward rounding bound). Image 0 of EVERY case has the planted
    extreme at (N - 1, M - 1): without the last key, and without the last row, its maximum (probe_neg) and its minimum (probe_pos) change."""
    scope = "head" if case.kernel == "scope_head_parts" else "image"
    pad_rows, pad_keys = case.N % 32 != 0, case.M % 32 != 0
    at_edge = {"last_key_excluded": set(), "last_row_excluded": set()}        # fields shown to move in image 0, per fault
    for variant in sc.DYADIC + ("shifted",):
        inp = sc.build(case, torch.float16, variant)
        s = sc.scores(inp["q"], inp["k"], case.H)
        f = sc.fields(s, scope)
        bar_sum, bar_sq = sc.sum_bars(s, variant, case, inp["q"], inp["k"])
        if variant != "shifted":
            other = sc.build(case, torch.bfloat16, variant)
            assert all(torch.equal(inp[n].double(), other[n].double()) for n in inp if torch.is_tensor(inp[n])), "inexact in a storage type"
            _check_exact(s)
            if case.kernel == "qproj_stat":
                assert torch.equal(inp["q"].double(), inp["x"].double() @ inp["w"].double().t())
                assert set(inp["q"].unique().tolist()) <= {0.5, 0.75, 0.875, 1.0, 1.25}
            D, neg = case.D, variant.endswith("neg")
            near_field, far_field = (0, 1) if neg else (1, 0)         # the field the near probe / a padding zero shows in
            sign = -1.0 if neg else 1.0
            if variant.startswith("probe"):
                assert bool((f[..., near_field] == sign * 0.25 * D).all())
            else:
                assert bool((f[..., 0] <= -0.5625 * D).all()) if neg else bool((f[..., 1] >= 0.5625 * D).all())
        for fault in sc.FAULTS:
            fe = sc.fields(sc.emulate(s, fault), scope)
            moved = fe != f
            dsum, dsq = (fe[..., 2] - f[..., 2]).abs(), (fe[..., 3] - f[..., 3]).abs()
            if fault == "padding_leak":
                if variant != "shifted" and (pad_rows or pad_keys):
                    assert bool(moved[..., near_field].all()), (variant, fault)
                continue
            if fault == "tail_rows_duplicated" and not pad_rows:
                continue
            assert bool((dsum > bar_sum).all()) and bool((dsq > bar_sq).all()), (variant, fault)
            if variant.startswith("probe") and fault != "tail_rows_duplicated":
                axis, last = (1, case.M - 1) if fault == "last_key_excluded" else (0, case.N - 1)
                assert bool(moved[0, ..., near_field].all()), (variant, fault)            # (unconditional: image 0 of every case)
                at_edge[fault].add(near_field)
                for b, (near, far) in enumerate(sc.probes(case)):
                    if near[axis] == last:
                        assert bool(moved[b, ..., near_field].all()), (variant, fault, b)
                    if far is not None and far[axis] == last:
                        assert bool(moved[b, ..., far_field].all()), (variant, fault, b)
    assert at_edge == {"last_key_excluded": {0, 1}, "last_row_excluded": {0, 1}}


def test_probe_cell_carries_the_extreme():
    """Without the near probe's cell the maximum of probe_neg falls from -0.25 D to the next score of a probe vector (<= -0.375 D)"""
    for name in ("qk_parts_b2h3n33m33d64", "long_qk_parts_b2h2n33m129d40", "qproj_stat_b2h8n70m33d40c128"):
        case = sc.BY_NAME[name]
        s = sc.scores(*(sc.build(case, torch.bfloat16, "probe_neg")[n] for n in ("q", "k")), case.H)
        for b, (near, _) in enumerate(sc.probes(case)):
            assert s[b].amax().item() == -0.25 * case.D
            s[b, :, near[0], near[1]] = -math.inf
            assert s[b].amax().item() <= -0.375 * case.D


def test_shifted_inputs_have_a_mean_far_from_zero():
    for name in ("qk_stats_b2h2n129m65d80", "qk_parts_b2h2n70m64d80_sharedk", "scope_head_parts_b2h3n33m32d64"):
        case = sc.BY_NAME[name]
        inp = sc.build(case, torch.float16, "shifted")
        s = sc.scores(inp["q"], inp["k"], case.H)
        assert abs(s.mean().item()) >= 2.0 * s.std().item() / math.sqrt(case.D) and abs(s.mean().item()) >= 0.15 * case.D
    assert sc.lane_chain(sc.BY_NAME["qk_stats_b2h2n63m129d96"]) == 96 and sc.lane_chain(sc.BY_NAME["qk_parts_b2h2n1m1d8"]) == 16


def test_views_sit_in_nan():
    case = sc.BY_NAME["qproj_stat_b2h8n70m77d40c128_sharedk"]
    inp = sc.build(case, torch.float16, "view")
    v = sc.as_views(inp)
    for n in ("q", "k", "x"):
        t = v[n]
        assert torch.equal(t, inp[n]) and not t.is_contiguous() and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0
        whole = torch.as_strided(t, (t.shape[0], t.shape[1] + sc.PAD_ROWS, t.shape[2] + sc.PAD_COLS), t.stride())
        assert bool(torch.isnan(whole[:, t.shape[1]:]).all()) and bool(torch.isnan(whole[:, :, t.shape[2]:]).all())
    assert v["k"].shape[0] == 1


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", sc.ROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_scope_oracle_shows_a_leak(shape, dtype):
    """A row maximum (neg) / minimum (pos) that is the padding's 0 instead of -+0.5625 D or beyond moves the oracle's output by at least 10 bars
    (TOL max|O|). stat_cases.row_oracle restates the oracle of test_scoped_stats_gpu.py; the GPU test compares the two."""
    B, H, N, M, D = shape
    assert M % 32 != 0
    for variant, kind in (("neg", "MAX"), ("pos", "MIN")):
        inp = sc.row_inputs(shape, dtype, variant)
        assert inp["scalar"] * 0.25 * D * inp["scale"] >= 2.0 - 1e-12 and bool((inp["w"][:, M - 1] > 0.8).any())
        ref, leaky = sc.row_oracle(inp, kind), sc.row_oracle(inp, kind, leak=True)
        bar = TOL[dtype] * ref.abs().max().item()
        print("%s %s %s: a leaking zero moves the oracle by %.0f bars" % (shape, variant, kind, (ref - leaky).abs().max().item() / bar))
        assert (ref - leaky).abs().max().item() >= 10 * bar


def test_synthetic_partials(libs):
    for P in sc.FOLD_COUNTS:
        parts = sc.synthetic_parts((2,), P, P)
        assert parts.shape == (2, P, 4) and torch.equal(parts[..., :2].float().double(), parts[..., :2])
        f = sc.fold(parts)
        assert bool((f[:, 0] == -0.5).all()) and bool((f[:, 1] == 0.25).all()) and bool((parts[:, :P - 1, 0] < -0.5).all()) and bool((parts[:, :P - 1, 1] > 0.25).all())
        neutral = torch.isinf(parts[..., 0])
        assert int(neutral[0].sum()) == len([i for i in range(P - 1) if i % 3 == 1]) and bool((parts[neutral][:, 2:] == 0).all())
        assert bool((parts[~neutral][:, 2] < 0).all())
    for P in sc.SCOPE_FOLD_COUNTS:
        assert _library_count(libs, "scope_head_parts", 1, 2, sc.scope_fold_rows(P), 5, 8) == P
    # the scope library never has more than 256 partials per (image, head)
    assert max(sc.model_scope_head_parts(1, 1, N, 5, 8)[1] for N in range(1, 200000, 997)) <= 256
    assert sc.FOLD_SHAPES["lean"][3] >= 64 and (sc.FOLD_SHAPES["lean"][3] + 15) // 16 * 16 <= 64 and sc.FOLD_SHAPES["general"][3] < 64
