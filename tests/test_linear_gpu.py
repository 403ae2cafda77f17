"""ops.linear (csrc/pww_linear.hip, libpww_hip_linear.so): the GEMM against an fp32 reference, its epilogues bit for bit against the unfused
sequence, repeatability, declines, and the routes of pww_hip.blocks that use it."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DEV = "cuda:0"


def _ops():
    from pww_hip import ops
    return ops


def _inputs(M, K, N, dtype, xs=None, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + M * 7 + K * 3 + N)
    xs = xs or K
    xbuf = torch.randn(M, xs, generator=g).to(DEV, dtype)
    x = xbuf[:, :K]
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV, dtype)
    b = (torch.randn(N, generator=g) * 0.5).to(DEV, dtype)
    return x, w, b


def _check(y, x, w, b, dtype, steps=2):
    """tests/test_conv_gpu.py::_check: |y - ref| <= 2 ULP (s + 1e-2 max s), s = |ref| without a bias, |acc| + |ref| with one."""
    acc = F.linear(x.float(), w.float())
    ref = acc + b.float() if b is not None else acc
    scale = acc.abs() + ref.abs() if b is not None else ref.abs()
    assert y.shape == ref.shape and y.dtype == dtype
    err = (y.float() - ref).abs()
    tol = steps * ULP[dtype] * (scale + 1e-2 * scale.max())
    print("max |err| %.3e, max |ref| %.3e, worst err / tol %.3f" % (err.max().item(), ref.abs().max().item(), (err / tol).max().item()))
    bad = err > tol
    assert not bad.any(), "%d of %d outside the bar; max |err| %.3e (max |ref| %.3e)" % (int(bad.sum()), bad.numel(), err.max().item(), ref.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 130, 257])
def test_against_fp32_reference(M, dtype):
    """M: the tail alone, less than a tile + tail, just over two tiles. K = 64 / 192 / 320: 1, 3 and 5 slabs (drain only; drain; the steady loop
    once). Both tile widths, splits 1 / 2 / 5 (2 and 5 leave splits shorter than 4 slabs), with and without a bias."""
    ops = _ops()
    for K, N in itertools.product((64, 192, 320), (64, 128, 320)):
        x, w, b = _inputs(M, K, N, dtype)
        for tn, sk in itertools.product((64, 128), (1, 2, 5)):
            if N % tn or sk > K // 64:
                continue
            _check(ops.linear(x, w, tile_n=tn, splitk=sk), x, w, None, dtype)
            _check(ops.linear(x, w, b, tile_n=tn, splitk=sk), x, w, b, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_row_stride_above_k(dtype):
    ops = _ops()
    x, w, b = _inputs(130, 192, 128, dtype, xs=192 + 24)
    assert x.stride(0) == 216 and not x.is_contiguous()
    for tn, sk in ((64, 1), (128, 3)):
        y = ops.linear(x, w, b, tile_n=tn, splitk=sk)
        _check(y, x, w, b, dtype)
        assert torch.equal(y, ops.linear(x.contiguous(), w, b, tile_n=tn, splitk=sk))


# (rows, K, N) of one feed-forward per level of the SD1.5 UNet at 2 rows: the GEGLU projection and the output linear
FF_SHAPES = [(8192, 320, 2560), (8192, 1280, 320), (2048, 640, 5120), (2048, 2560, 640), (512, 1280, 10240), (512, 5120, 1280), (128, 1280, 10240), (128, 5120, 1280)]


@pytest.mark.parametrize("shape", FF_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_feed_forward_shapes_two_rows(shape):
    """The real shapes at the library's own tile / split choice: the projection with GEGLU against ops.geglu of the biased GEMM (exact) and
    the fp32 reference, the output linear with its residual."""
    from pww_hip import _lib
    ops = _ops()
    M, K, N = shape
    geglu = N == 8 * K
    x, w, b = _inputs(M, K, N, torch.bfloat16)
    # the split the library plans for the fused call (the tile width does not change the order of the sum, the split does)
    d = _lib.LinearDesc(ctypes.sizeof(_lib.LinearDesc), _lib.DTYPE_BF16, M, N, K, _lib.LINEAR_BIAS_GEGLU if geglu else _lib.LINEAR_BIAS_RESIDUAL, 0, 0, 0, 0, 0)
    split = max(1, _lib.load_linear().pww_linear_workspace_bytes(ctypes.byref(d)) // (4 * M * N))
    y = ops.linear(x, w, b, splitk=split)
    _check(y, x, w, b, torch.bfloat16)
    if geglu:
        assert torch.equal(ops.linear(x, w, b, geglu=True), ops.geglu(y))
    else:
        r = torch.randn(M, N, device=DEV).to(torch.bfloat16)
        assert torch.equal(ops.linear(x, w, b, residual=r), (r.float() + y.float()).to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_epilogues_exact(dtype):
    """BIAS = T(T(acc) + b): equal to (plain.float() + b).to(T) for ANY split, provided plain and biased call use the same (tile_n, split) --
    the fold sums the fp32 partials in split order and then applies the same epilogue code. BIAS_RESIDUAL and BIAS_GEGLU restate the unfused
    sequence on the biased result.
    GEGLU in fp16 is compared within ONE fp16 ULP instead of bit for bit: hipcc builds pww_geglu's fp16 code object with v_fma_mixlo_f16, which
    rounds the fp32 product 0.5 g (1 + erf) to fp16 ONCE, where this kernel's code object (like ATen's F.gelu) rounds it to fp32 and then to
    fp16; the two differ by one ULP on the rare product that sits on a double-rounding boundary: the fp32 rounding has to land within 2^-13
    of its spacing of an fp16 midpoint, about 1e-4 of the elements, so at most 1e-3 of them may differ, and none by more than that ULP.
    The same source line compiles to the same instructions for bf16, where the comparison is exact."""
    ops = _ops()
    for (M, K, N), tn, sk in itertools.product(((130, 192, 128), (257, 320, 384)), (64, 128), (1, 2, 3)):
        x, w, b = _inputs(M, K, N, dtype)
        plain = ops.linear(x, w, tile_n=tn, splitk=sk)
        with_bias = ops.linear(x, w, b, tile_n=tn, splitk=sk)
        assert torch.equal(with_bias, (plain.float() + b.float()).to(dtype))
        rbuf = torch.randn(M, N + 8, device=DEV).to(dtype)
        r = rbuf[:, :N]                                                        # (its own row stride)
        want = (r.float() + with_bias.float()).to(dtype)
        assert torch.equal(ops.linear(x, w, b, residual=r, tile_n=tn, splitk=sk), want)
        alias = r.contiguous()
        assert ops.linear(x, w, b, residual=alias, out=alias, tile_n=tn, splitk=sk) is alias and torch.equal(alias, want)      # y aliases r
        inner = N // 2                                                          # 64 and 192
        want = ops.geglu(with_bias)
        got = ops.linear(x, w, b, geglu=True, tile_n=tn, splitk=sk)
        if dtype == torch.bfloat16:
            assert torch.equal(got, want)
        else:
            d = (got.float() - want.float()).abs()
            print("fp16 GEGLU: %d of %d elements differ from pww_geglu" % (int((d > 0).sum()), d.numel()))
            assert bool((d <= ULP[dtype] * 2 * want.float().abs().clamp_min(2.0 ** -14)).all()) and int((d > 0).sum()) * 1000 <= d.numel()
        want = got
        obuf = torch.full((M, inner + 16), 7.0, device=DEV, dtype=dtype)
        out = ops.linear(x, w, b, geglu=True, tile_n=tn, splitk=sk, out=obuf[:, :inner])          # output row stride above inner
        assert torch.equal(out, want) and bool((obuf[:, inner:] == 7.0).all())


@pytest.mark.parametrize("sk", [1, 3], ids=["nosplit", "split3"])
def test_repeatable(sk):
    ops = _ops()
    x, w, b = _inputs(257, 320, 384, torch.bfloat16)
    r = torch.randn(257, 384, device=DEV).to(torch.bfloat16)
    calls = [lambda: ops.linear(x, w, b, residual=r, splitk=sk), lambda: ops.linear(x, w, b, geglu=True, splitk=sk)]
    for call in calls:
        first = call()
        assert all(torch.equal(first, call()) for _ in range(2))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = call()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(first, y)


def test_declines():
    """K or N off the 64 grid, fp32 and an odd inner: the library answers PWW_ENOTSUP, ops.linear raises, and the route keeps the stock GEMM
    and says so in the `linear` counter."""
    from pww_hip import _lib, blocks
    ops = _ops()
    lib = _lib.load_linear()
    for M, N, K, epi in ((16, 64, 72, 0), (16, 72, 64, 0), (16, 192, 64, 3)):
        d = _lib.LinearDesc(ctypes.sizeof(_lib.LinearDesc), _lib.DTYPE_BF16, M, N, K, epi, 0, 0, 0, 0, 0)
        t = torch.zeros(M * max(N, K), device=DEV, dtype=torch.bfloat16)
        rc = lib.pww_linear_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), None, t.data_ptr(), ctypes.byref(d), None, 0, None)
        assert rc == _lib.PWW_ENOTSUP and lib.pww_linear_workspace_bytes(ctypes.byref(d)) == 0
    cases = [(torch.randn(16, 72), torch.randn(64, 72), False, torch.bfloat16), (torch.randn(16, 64), torch.randn(72, 64), False, torch.bfloat16),
             (torch.randn(16, 64), torch.randn(64, 64), False, torch.float32), (torch.randn(16, 64), torch.randn(192, 64), True, torch.bfloat16)]
    old = blocks.LINEAR
    blocks.LINEAR = "force"
    try:
        for x, w, geglu, dt in cases:
            x, w = x.to(DEV, dt), w.to(DEV, dt)
            b = torch.zeros(w.shape[0], device=DEV, dtype=dt)
            assert not ops.linear_takes(x, w, geglu)
            with pytest.raises(ops.PwwHipError):
                ops.linear(x, w, b, geglu=geglu)
            blocks.reset_stats()
            assert not blocks._linear_route(x, w, b, "geglu" if geglu else "residual")
            assert blocks.stats()["linear"] == {"fused": 0, "declined": 1}
        # operands the library answers PWW_EINVAL to decline as well: a bias off the 8-byte grid, a residual whose row pitch is no multiple of 8
        x, w, b = _inputs(16, 64, 64, torch.bfloat16)
        b_off = torch.cat([b[:1], b])[1:]
        r_odd = torch.zeros(16, 68, device=DEV, dtype=torch.bfloat16)[:, :64]
        assert b_off.data_ptr() % 8 != 0 and b_off.is_contiguous() and r_odd.stride(0) % 8 != 0
        blocks.reset_stats()
        assert blocks._linear_route(x, w, b, "residual", residual=torch.zeros_like(r_odd).contiguous())
        assert not blocks._linear_route(x, w, b_off, "residual") and not blocks._linear_route(x, w, b, "residual", residual=r_odd)
        assert blocks.stats()["linear"] == {"fused": 1, "declined": 2}
        assert torch.equal(ops.linear(x, w, b_off, residual=r_odd), ops.linear(x, w, b))          # (ops.linear itself copies what it has to)
    finally:
        blocks.LINEAR = old
        blocks.reset_stats()


def _block_and_model(dtype):
    import sd_standin.unet as U
    torch.manual_seed(3)
    blk = U.BasicTransformerBlock(128, 2, 64, 96).to(DEV, dtype).eval()           # 1/8 of the widths 1024 / 768: inner 128, ff 512
    tm = U.Transformer2DModel(2, 64, 128, 96).to(DEV, dtype).eval()
    return blk, tm


def _capture(mods):
    """Forward hooks that keep (input, output) of each module in `mods` (name -> module) in fp32."""
    seen, handles = {}, []
    for name, m in mods.items():
        handles.append(m.register_forward_hook(lambda mod, inp, out, name=name: seen.__setitem__(name, (inp[0].float(), out.float()))))
    return seen, handles


K_ROUTE = 5


def _route_bar(s, moved, weight, u):
    """The bar of `_check` for an output y = T(a + T(acc + b)) whose two routes round differently: |err| <= K_ROUTE u (s + 1e-2 max s) with
    s = |a| + |T(acc + b)|, the magnitudes that meet at the last rounding point (u = ULP[dtype], the half-spacing). K_ROUTE counts the
    roundings of relative size u that separate the routes there: y once per route (2, each at most u |y| <= u s) and the GEMM's output once
    on the stock route, T(acc + b), and twice on the HIP route, T(T(acc) + b) (3, each at most u s up to the bias, which the floor covers).
    On top comes what no rounding at s carries: the GEMM's INPUT differs between the routes, each element by at most about one spacing of
    its own rounding (`moved` = 2 u |input|), with no preferred sign, so acc moves like a random sum: 4 sigma of it,
    4 sqrt(sum_j moved_j^2 w_ij^2) -- the root of the sum of squares, not the sum of magnitudes."""
    walk = 4 * F.linear(moved * moved, weight.float() ** 2).sqrt()
    return K_ROUTE * u * (s + 1e-2 * s.max()), walk


def test_routes_through_blocks():
    """A 1/8-width BasicTransformerBlock and Transformer2DModel under install_blocks: with the route table forced to the HIP kernel the output
    stays within the 2-ULP-class bar of the same modules under PWW_LINEAR=0 (`_route_bar`), and stats() shows the calls. Block: y = h + v,
    v the feed-forward's output linear, whose input g (the GEGLU output) is rounded differently by the two routes. Transformer2DModel:
    y = proj_out + residual, proj_out the same GEMM in both routes on the block's output. A bar in |y| alone would be wrong: h + v cancels."""
    from pww_hip import blocks
    dtype = torch.bfloat16
    u = ULP[dtype]
    blk, tm = _block_and_model(dtype)
    blocks.install_blocks(tm)
    holder = torch.nn.ModuleList([blk])
    blocks.install_blocks(holder)
    x = torch.randn(2, 130, 128, device=DEV).to(dtype)
    ctx = torch.randn(2, 77, 96, device=DEV).to(dtype)
    img = torch.randn(2, 128, 12, 11, device=DEV).to(dtype)
    old = blocks.LINEAR
    try:
        with torch.no_grad():
            blocks.LINEAR = "0"
            blocks.reset_stats()
            tblk = tm.transformer_blocks[0]
            seen_b, hb = _capture({"out": blk.ff.net[2]})
            seen_t, ht = _capture({"blk": tblk, "proj_out": tm.proj_out})
            try:
                ref_b, ref_t = blk(x, context=ctx), tm(img, encoder_hidden_states=ctx)
            finally:
                for h in hb + ht:
                    h.remove()
            assert blocks.stats()["linear"] == {"fused": 0, "declined": 2}          # (the two GEGLU projections, counted as declined)
            g, v = seen_b["out"]
            h = ref_b.float() - v                                    # (the sum's other operand, to within the rounding of y: u |y| of s)
            bar_b = _route_bar(h.abs() + v.abs(), 2 * u * g.abs(), blk.ff.net[2].weight, u)
            p = seen_t["proj_out"][1]                                  # [2, 128, 12, 11]
            wp = tm.proj_out.weight.reshape(tm.proj_out.out_channels, -1)
            moved = 2 * u * seen_t["blk"][1].abs()                     # [2, 132, 128]: one spacing of the block's output
            floor_t, walk_t = _route_bar(p.abs() + img.float().abs(), moved, wp, u)
            bar_t = floor_t, walk_t.reshape(2, 12, 11, -1).permute(0, 3, 1, 2)
            blocks.LINEAR = "force"
            blocks.reset_stats()
            y_b = blk(x, context=ctx)
            s = blocks.stats()
            assert s["linear"] == {"fused": 2, "declined": 0} and s["geglu"]["fused"] == 1 and s["transformer_block"]["fused"] == 1 and s["hit_rate"] == 1.0
            y_t = tm(img, encoder_hidden_states=ctx)
            assert blocks.stats()["linear"]["fused"] == 4
            blocks.LINEAR = "1"                                  # the table: these widths are not in it
            blocks.reset_stats()
            assert torch.equal(blk(x, context=ctx), ref_b) and blocks.stats()["linear"] == {"fused": 0, "declined": 2}
            # a call outside the restated signature reaches the module's own forward with its arguments as given
            blocks.LINEAR = "force"
            blocks.reset_stats()
            geglu = blk.ff.net[0]
            own = geglu.__dict__["_pww_orig_forward"]
            geglu.__dict__["_pww_orig_forward"] = lambda *a, **k: ("own", a, k)
            try:
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = geglu(x, scale=0.5)
            finally:
                geglu.__dict__["_pww_orig_forward"] = own
            assert got[0] == "own" and got[1][0] is x and got[2] == {"scale": 0.5}
            assert blocks.stats()["linear"] == {"fused": 0, "declined": 0} and blocks.stats()["geglu"] == {"fused": 0, "declined": 1}
    finally:
        blocks.LINEAR = old
        blocks.reset_stats()
        blocks.uninstall_blocks(tm)
        blocks.uninstall_blocks(holder)
    for name, y, ref, (tol, walk) in (("block", y_b, ref_b, bar_b), ("Transformer2DModel", y_t, ref_t, bar_t)):
        err = (y.float() - ref.float()).abs()
        print("route %s: max |err| %.3e, max |ref| %.3e, median K u (s + 1e-2 max s) %.3e, median walk term %.3e, worst err / bar %.3f, %d of %d elements differ"
              % (name, err.max().item(), ref.float().abs().max().item(), tol.median().item(), walk.median().item(), (err / (tol + walk)).max().item(),
                 int((err > 0).sum()), err.numel()))
        assert y.shape == ref.shape and not (err > tol + walk).any()
