"""Every launch form of pww_group_norm_fwd (csrc/pww_norm.hip) and the edges of the elementwise kernels beside it (csrc/pww_blocks.hip),
through pww_hip.ops, against the fp32 / fp64 reference of tests/norm_cases.py and the stock op sequence on the same GPU.

test_norm_gpu.py runs these kernels at the SD shapes with 32 groups. Here (shape table and its comments: norm_cases.GN_CASES): the
512-thread two-launch NHWC form, group counts 1 / 3 / 5 / 8 / 24 / 28 (fold lanes that idle, chunks that straddle groups), 1024 and 257
channels per group, the NCHW single-launch form with several chunks per row and thread, both sides of the single- / two-launch boundary
in both layouts, tensors smaller than the single-launch form's pixels in flight, `pre_bias` alone and with `add`, every combination of
the optional operands, caller-supplied workspaces, and float16 statistics under a mean of 600 spreads. tests/test_norm_cases_host.py
holds the reference to the stock CPU sequence at the same shapes and the table's forms to the library's own plan.

Bars (norm_cases.close; the bars of test_norm_gpu.py): one rounding step of the storage type against the reference, two behind SiLU, no
element outside; two steps relative to the tensor's maximum against the stock sequence.

One-line changes of a kernel that a case here turns into a failure, argued from the code:
  any of the six       `if (p.pre)` dropped, or `pre` added after `add`: every (pre, *) variant (pre moves a value by hundreds of steps; the
                       order of the two roundings by one).
  gn_moments_nhwc      `g = tid & 31` for `tid % p.G`: every G other than 32. `p1` without the clamp to HW: (2, 16, 104, 104, 1), whose last
                       slab holds 576 of 1024 pixels, takes image 1's pixels into image 0's sums.
  gn_apply_nhwc<512>   `PL = 256 / CH`: 0 at C = 2560, no thread is active and y stays unwritten.
  gn_group_nhwc        `ok` taken from piece 0: (1, 320, 8, 74, 8), where piece 23 holds 17 of 25 pixels and the clamped loads repeat piece 0.
  gn_group_nchw        `kper = cpr / TPR`: (1, 16, 48, 64, 8), 384 chunks per row on 256 threads, loses the chunks 256 .. 383.
  f16 statistics       the pivot not added back (`n * c` dropped from the sum): every float16 case, by the mean."""
import pytest
import torch
import torch.nn.functional as F

import norm_cases as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)  # noqa: E731


def _ops():
    from pww_hip import ops
    return ops


def _to_dev(t, channels_last=False):
    t = t.to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


def _check(ops, x, G, w, b, eps, add, pre, act, dtype, what, **kw):
    """One call against the reference and the stock sequence; returns the output."""
    y = ops.group_norm(x, G, w, b, eps, add=add, act=act, pre_bias=pre, **kw)
    assert y.shape == x.shape and y.stride() == x.stride() and y.dtype == dtype, what
    ref = N.reference(x, add, w, b, G, eps, act, dtype, pre=pre)
    nbad, rel = N.close(y, ref, dtype, steps=2 if act else 1)
    print("%s: %d outside, max err / max = %.3e" % (what, nbad, rel))
    assert nbad == 0, (what, nbad, rel)
    rel2 = N.close(y, N.stock(x, add, w, b, G, eps, act, pre=pre), dtype)[1]
    assert rel2 <= 2 * N.ULP[dtype], ("vs stock", what, rel2)
    return y


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=_ids)
def test_group_norm_forms_and_addends(shape, channels_last, dtype):
    ops = _ops()
    G = shape[4]
    x, w, b, add, pre = N.gn_inputs(shape, dtype)
    x, w, b, add, pre = _to_dev(x, channels_last), _to_dev(w), _to_dev(b), _to_dev(add), _to_dev(pre)
    for use_pre, use_add in N.ADDENDS:
        for act in N.ACTS:
            _check(ops, x, G, w, b, 1e-5, add if use_add else None, pre if use_pre else None, act, dtype,
                   (shape, channels_last, dtype, "pre" if use_pre else "-", "add" if use_add else "-", act))
    # the addend as rows of a wider tensor: no copy, same bits
    B, C = shape[:2]
    wide = torch.zeros(B, C + 64, device=DEV, dtype=dtype)
    wide[:, 32:32 + C] = add
    assert torch.equal(ops.group_norm(x, G, w, b, 1e-5, add=wide[:, 32:32 + C], act="silu", pre_bias=pre),
                       ops.group_norm(x, G, w, b, 1e-5, add=add, act="silu", pre_bias=pre))


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
@pytest.mark.parametrize("shape,channels_last", N.AFFINE_CASES, ids=_ids)
def test_group_norm_without_weight_or_bias(shape, channels_last, dtype):
    ops = _ops()
    x, w, b, add, pre = N.gn_inputs(shape, dtype)
    x, w, b, add, pre = _to_dev(x, channels_last), _to_dev(w), _to_dev(b), _to_dev(add), _to_dev(pre)
    for use_w, use_b in N.AFFINE:
        for act in N.ACTS:
            _check(ops, x, shape[4], w if use_w else None, b if use_b else None, 1e-5, add, pre, act, dtype,
                   (shape, channels_last, dtype, "w" if use_w else "-", "b" if use_b else "-", act))


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_group_norm_in_place_on_the_two_launch_form(channels_last):
    ops = _ops()
    dtype = torch.bfloat16
    x, w, b, add, pre = N.gn_inputs(N.IN_PLACE, dtype)
    x, w, b, add, pre = _to_dev(x, channels_last), _to_dev(w), _to_dev(b), _to_dev(add), _to_dev(pre)
    y = ops.group_norm(x, N.IN_PLACE[4], w, b, 1e-5, add=add, act="silu", pre_bias=pre)
    x2 = x.clone(memory_format=torch.preserve_format)
    assert ops.group_norm(x2, N.IN_PLACE[4], w, b, 1e-5, add=add, act="silu", pre_bias=pre, out=x2) is x2 and torch.equal(x2, y)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", [(2, 2560, 24, 24, 32), (2, 16, 104, 104, 1), (1, 320, 19, 32, 8), (2, 96, 5, 8, 24)], ids=_ids)
def test_group_norm_workspace_from_the_caller(shape, channels_last):
    """A workspace of 0xFF bytes (NaN partials wherever the kernels read what they did not write) gives the bits of a fresh one -- "no
    state that must be zero" -- and one a byte short is refused before anything is launched."""
    import ctypes
    from pww_hip import PwwHipError, _lib
    ops = _ops()
    dtype = torch.float16
    B, C, H, W, G = shape
    x, w, b, add, pre = N.gn_inputs(shape, dtype)
    x, w, b, add, pre = _to_dev(x, channels_last), _to_dev(w), _to_dev(b), _to_dev(add), _to_dev(pre)
    d = _lib.GnDesc(_lib.DTYPE_F16, _lib.LAYOUT_NHWC if channels_last else _lib.LAYOUT_NCHW, B, C, H * W, G, 1e-5, _lib.ACT_SILU, C, 0)
    need = int(_lib.load().pww_group_norm_workspace_bytes(ctypes.byref(d)))
    assert need >= 16
    y = ops.group_norm(x, G, w, b, 1e-5, add=add, act="silu", pre_bias=pre)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    assert torch.equal(ops.group_norm(x, G, w, b, 1e-5, add=add, act="silu", pre_bias=pre, workspace=ws), y)
    with pytest.raises(PwwHipError):
        ops.group_norm(x, G, w, b, 1e-5, add=add, act="silu", pre_bias=pre, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


# ---- statistics under a large mean --------------------------------------------------------------------------------------------------------
_NOISE = {}


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("mean,sigma", N.STAT_REGIMES)
@pytest.mark.parametrize("shape", N.STAT_SHAPES, ids=_ids)
def test_group_norm_statistics_under_a_large_mean(shape, mean, sigma, channels_last, dtype):
    """No affine, eps 1e-6: the output is (h - mean) * rstd, so a relative error of rstd is a relative error of every output. One step.
    One shape per accumulating kernel; mean 300 / sigma 0.5 is where plain fp32 sums of float16 squares break (csrc/pww_norm.hip, header),
    30 / 0.5 and 60 / 1.0 what the workload can reach. bfloat16 cannot fail through the sums (test_norm_cases_host.py says why): its
    cases hold the rest of the arithmetic at these magnitudes."""
    ops = _ops()
    if shape not in _NOISE:
        _NOISE[shape] = N.stat_noise(shape).to(DEV)
    x = (mean + sigma * _NOISE[shape]).to(dtype)
    x = x.contiguous(memory_format=torch.channels_last) if channels_last else x
    G = shape[4]
    y = ops.group_norm(x, G, None, None, 1e-6)
    ref = N.reference(x, None, None, None, G, 1e-6, None, dtype)
    yf, rf = y.float(), ref.float()
    tol = N.ULP[dtype] * (rf.abs() + 1e-2 * rf.abs().max())
    worst = float(((yf - rf).abs() / tol).max())
    nbad = N.close(y, ref, dtype)[0]
    print("large mean %s mean %g sigma %g %s %s: %d outside, worst err / tol %.3f"
          % (_ids(shape), mean, sigma, "nhwc" if channels_last else "nchw", dtype, nbad, worst))
    assert nbad == 0, (shape, mean, sigma, channels_last, dtype, nbad, worst)


# ---- add + LayerNorm ----------------------------------------------------------------------------------------------------------------------
def _ln_ref(s, w, b, eps, dtype, double=False):
    f = (lambda t: None if t is None else t.double()) if double else (lambda t: None if t is None else t.float())
    return F.layer_norm(f(s), (s.shape[-1],), f(w), f(b), eps).to(dtype)


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
@pytest.mark.parametrize("C", N.LN_CHANNELS)
def test_add_layer_norm_at_the_template_boundaries(C, dtype):
    """plain, add and add + post_bias at every C next to a change of the chunks-per-lane template, 1 and 5 rows (a workgroup holds 4),
    weight and bias each present or None, strided a and x: s bit-equal to the stock adds, y within one step of an fp32 LayerNorm of s."""
    ops = _ops()
    for rows in N.LN_ROWS:
        x, a, w, b, pb = (t.to(DEV) for t in N.ln_inputs(rows, C, dtype))
        s_want = a + x
        for use_w in (True, False):
            for use_b in (True, False):
                ww, bb = w if use_w else None, b if use_b else None
                what = (rows, C, dtype, use_w, use_b)
                ref = _ln_ref(s_want, ww, bb, 1e-5, dtype)
                s, y = ops.add_layer_norm(x, ww, bb, 1e-5, a=a)
                assert torch.equal(s, s_want), what
                assert N.close(y, ref, dtype)[0] == 0, what
                assert torch.equal(ops.add_layer_norm(s_want, ww, bb, 1e-5), y), what                 # plain form: same arithmetic
                s3, y3 = ops.add_layer_norm(x, ww, bb, 1e-5, a=a, post_bias=pb)
                assert torch.equal(s3, s_want + pb) and torch.equal(y3, y), what                     # the norm is that of a + x
        wide_x = torch.zeros(rows, C + 24, device=DEV, dtype=dtype)
        wide_a = torch.zeros(rows, C + 40, device=DEV, dtype=dtype)
        wide_x[:, 8:8 + C] = x
        wide_a[:, 16:16 + C] = a
        s, y = ops.add_layer_norm(x, w, b, 1e-5, a=a, post_bias=pb)
        s2, y2 = ops.add_layer_norm(wide_x[:, 8:8 + C], w, b, 1e-5, a=wide_a[:, 16:16 + C], post_bias=pb)
        assert torch.equal(s2, s) and torch.equal(y2, y), (rows, C, dtype, "strided")


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
def test_add_layer_norm_statistics_survive_a_large_mean(dtype):
    """mean 300, sigma 0.5 at C = 1288: the kernel takes the mean first and sums centred squares, so one step of an fp64 LayerNorm holds."""
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(1288)
    x = (300.0 + 0.5 * torch.randn(5, 1288, generator=g)).to(DEV, dtype)
    y = ops.add_layer_norm(x, None, None, 1e-6)
    assert N.close(y, _ln_ref(x, None, None, 1e-6, dtype, double=True), dtype)[0] == 0


def test_add_layer_norm_declines():
    from pww_hip import PwwHipError
    ops = _ops()
    for C in N.LN_REFUSED:
        x = torch.zeros(2, C, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(PwwHipError):
            ops.add_layer_norm(x, None, None, 1e-5)
        with pytest.raises(PwwHipError):
            ops.add_layer_norm(x, None, None, 1e-5, a=x)
    x = torch.zeros(2, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(PwwHipError):
        ops.add_layer_norm(x, None, None, 1e-5, post_bias=torch.zeros(64, device=DEV, dtype=torch.bfloat16))


# ---- GEGLU --------------------------------------------------------------------------------------------------------------------------------
def _geglu_check(ops, h, dtype):
    y = ops.geglu(h)
    xa, gate = h.chunk(2, dim=-1)
    stock = xa * F.gelu(gate)
    ref = (xa.float() * F.gelu(gate.float()).to(dtype).float()).to(dtype)
    assert y.shape == stock.shape and y.is_contiguous()
    assert N.close(y, ref, dtype)[0] == 0 and N.close(y, stock, dtype)[0] == 0


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
def test_geglu_smallest_rows_and_a_row_stride(dtype):
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(16)
    for shape in ((1, 16), (1, 48)):
        _geglu_check(ops, (torch.randn(shape, generator=g) * 1.5).to(DEV, dtype), dtype)
    # a column slice of a wider tensor: row stride 2 D + 16, the neighbours hold NaN
    for rows, D in ((3, 24), (7, 320)):
        wide = torch.full((rows, 2 * D + 16), float("nan"), device=DEV, dtype=dtype)
        h = wide[:, 8:8 + 2 * D]
        h.copy_((torch.randn((rows, 2 * D), generator=g) * 1.5).to(DEV, dtype))
        assert h.stride(0) == 2 * D + 16
        _geglu_check(ops, h, dtype)
        assert torch.equal(ops.geglu(h), ops.geglu(h.contiguous()))
    from pww_hip import PwwHipError
    for width in (20, 24):                       # D = 10 and 12: no multiple of 8
        with pytest.raises(PwwHipError):
            ops.geglu(torch.zeros(2, width, device=DEV, dtype=dtype))


@pytest.mark.parametrize("dtype", N.DTYPES, ids=str)
def test_geglu_past_the_grid_cap(dtype):
    """4100 x 8192: 4 198 400 chunks against the 4096 x 256 x 4 = 4 194 304 of one trip of the capped grid -- the loop's second trip,
    nearly all of it masked."""
    torch.manual_seed(41)
    h = torch.randn(4100, 2 * 8192, device=DEV, dtype=dtype) * 1.5
    _geglu_check(_ops(), h, dtype)


# ---- bias + residual ------------------------------------------------------------------------------------------------------------------------
def test_bias_residual_nhwc_with_an_odd_plane():
    """channels_last with H * W no multiple of 8 (9 and 5 pixels): accepted in that layout, bit for bit the stock expression."""
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(33)
    for dtype in N.DTYPES:
        for shape in ((2, 8, 3, 3), (1, 24, 1, 5)):
            r = torch.randn(shape, generator=g).to(DEV, dtype).contiguous(memory_format=torch.channels_last)
            v = torch.randn(shape, generator=g).to(DEV, dtype).contiguous(memory_format=torch.channels_last)
            bias = torch.randn(shape[1], generator=g).to(DEV, dtype)
            y = ops.bias_residual(r, v, bias)
            assert y.shape == v.shape and y.stride() == v.stride() and torch.equal(y, r + (v + bias[None, :, None, None]))


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_bias_residual_past_the_grid_cap(channels_last):
    """(9, 64, 256, 256): 4 718 592 chunks against the 4 194 304 of one trip of the capped grid."""
    ops = _ops()
    torch.manual_seed(9)
    dtype = torch.bfloat16
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    r = torch.randn((9, 64, 256, 256), device=DEV, dtype=dtype).contiguous(memory_format=fmt)
    v = torch.randn((9, 64, 256, 256), device=DEV, dtype=dtype).contiguous(memory_format=fmt)
    bias = torch.randn(64, device=DEV, dtype=dtype)
    y = ops.bias_residual(r, v, bias)
    assert y.stride() == v.stride() and torch.equal(y, r + (v + bias[None, :, None, None]))
