"""The shape table and the reference of the norm kernels' GPU tests (tests/norm_cases.py), checked without a device.

test_norm_edges_gpu.py holds the kernels of csrc/pww_norm.hip to norm_cases.reference at shapes picked for the launch form they take.
Here the form each row of the table names is asked of the library's own plan (pww_group_norm_workspace_bytes runs no device code), and
the reference is held to the stock CPU sequence -- the adds on tensors of the storage type, F.group_norm in fp32, SiLU -- by the bars
the GPU tests use, at every shape and variant. CPU only."""
import ctypes

import pytest
import torch

import norm_cases as N

_ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)  # noqa: E731


def test_rows_take_the_form_the_table_names(built_lib):
    """16 bytes: the single-launch form (nothing is read from them); otherwise B * nslab * G partials of 16 bytes. A two-launch row with
    ONE partial answers 16 as well, so it says nothing about the form and is left out: (1, 4096, 2, 4, 1) in NHWC carries no form for that
    reason, (1, 1024, 4, 6, 1) in NCHW is skipped here."""
    from pww_hip import _lib
    lib = _lib.load()
    asked = 0
    for dtype in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
        for (B, C, H, W, G), nhwc, nchw in N.GN_CASES:
            for layout, form in ((_lib.LAYOUT_NHWC, nhwc), (_lib.LAYOUT_NCHW, nchw)):
                d = _lib.GnDesc(dtype, layout, B, C, H * W, G, 1e-5, _lib.ACT_NONE, 0, 0)
                got = lib.pww_group_norm_workspace_bytes(ctypes.byref(d))
                assert got >= 16, ((B, C, H, W, G), layout, "refused")
                if form is None or (form != "group" and B * form[1] * G == 1):
                    continue
                assert got == (16 if form == "group" else B * form[1] * G * 16), ((B, C, H, W, G), layout, form, got)
                asked += 1
    assert asked == 2 * (2 * len(N.GN_CASES) - 7)
    # what the table's comments say about the shapes themselves
    small = [s for s, nhwc, _ in N.GN_CASES if nhwc == "group" and s[2] * s[3] < 256 // (s[1] // s[4] // 4)]
    assert small == [(2, 8, 8, 1, 1), (2, 48, 6, 4, 3), (2, 96, 5, 8, 24), (3, 40, 8, 9, 5)]          # HW < PLs on the single-launch NHWC form
    assert sorted({s[4] for s in N.GN_SHAPES}) == [1, 3, 5, 8, 24, 28, 32]
    assert all(s in N.GN_SHAPES for s, _ in N.AFFINE_CASES) and N.IN_PLACE in N.GN_SHAPES


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=_ids)
def test_reference_matches_the_stock_cpu_sequence(shape, dtype):
    """One step, two behind SiLU, no element outside; two steps relative to the maximum: the bars the kernels are held to."""
    G = shape[4]
    x, w, b, add, pre = N.gn_inputs(shape, dtype)
    variants = [(w, b, add if use_add else None, pre if use_pre else None, act) for use_pre, use_add in N.ADDENDS for act in N.ACTS]
    if any(shape == s for s, _ in N.AFFINE_CASES):
        variants += [(w if use_w else None, b if use_b else None, add, pre, act) for use_w, use_b in N.AFFINE for act in N.ACTS]
    for ww, bb, aa, pp, act in variants:
        ref = N.reference(x, aa, ww, bb, G, 1e-5, act, dtype, pre=pp)
        want = N.stock(x, aa, ww, bb, G, 1e-5, act, pre=pp, norm_in_fp32=True)
        nbad, rel = N.close(ref, want, dtype, steps=2 if act else 1)
        what = (shape, dtype, ww is not None, bb is not None, aa is not None, pp is not None, act)
        assert nbad == 0 and rel <= 2 * N.ULP[dtype], (what, nbad, rel)


def test_large_mean_inputs_and_why_bfloat16_sums_are_exact():
    """The inputs of test_group_norm_statistics_under_a_large_mean are what they claim, and the arithmetic behind its docstring.

    A bfloat16 value has 8 significant bits, its square 16. The kernels add at most 96 values, or 96 squares, in fp32 before they go on in
    fp64; under a large mean those terms share one binade, so a partial sum needs at most 16 + 7 = 23 bits below its leading one and
    fp32's 24 hold it: the sums are exact, and bfloat16 statistics cannot lose accuracy to the mean. A float16 value has 11 bits, its
    square 22: from the fourth same-magnitude square on the fp32 sum rounds, and under mean 300 / sigma 0.5 the rounding errors are of
    the size of the variance. Hence the pivot of the f16 instantiations (csrc/pww_norm.hip, header)."""
    z = N.stat_noise(N.STAT_SHAPES[0])
    for mean, sigma in N.STAT_REGIMES:
        for dtype, bits in ((torch.bfloat16, 16), (torch.float16, 22)):
            x = (mean + sigma * z).to(dtype)
            assert abs(float(x.float().mean()) - mean) < 0.02 * mean and x.float().std() > 0.5 * sigma
            run = x.float().reshape(-1)[:96]
            sq = run * run
            # the squares are exact in fp32 (<= 22 bits) ...
            assert torch.equal(sq.double(), run.double() * run.double())
            # ... and 96 of them sum exactly in fp32 when they have 16 bits; with 22 the fp32 sum differs from the exact one
            s32 = torch.zeros((), dtype=torch.float32)
            for v in sq:
                s32 = s32 + v
            exact = float(s32.double()) == float(sq.double().sum())
            if bits == 16:
                assert exact, (mean, sigma, dtype)
            elif mean == 300.0:
                assert not exact, (mean, sigma, dtype)
