"""Per-head / per-row score statistics, host side (no GPU): the algebra that keeps `c * w * g(sigma) * qk.amax(dim=(1, 2), keepdim=True)` and
`... * qk.std(dim=-1, keepdim=True)` symbolic, every spelling that must stay on the materialised route, the third library (built, exports,
argument validation in front of the first HIP call, ISA) and the pin of the two weight functions to the reference's `inj_forward`."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pww_cases as cases
from oracle import pww_oracle as O

G = cases.GOLDEN


def wf_head(w, s, qk):
    return 0.4 * w * math.log(1 + s) * qk.amax(dim=(1, 2), keepdim=True)


def wf_row(w, s, qk):
    return 0.5 * w * math.log(1 + s ** 2) * qk.std(dim=-1, keepdim=True)


@pytest.fixture(scope="module")
def scope_lib_path(built_lib):
    import build as pww_build
    return pww_build.build_scope()


def _proxy(monkeypatch, B=2, H=2, N=6, M=5, D=8, seed=0):
    """A QKProxy over CPU tensors (the GEMM of _materialize runs on them) and the real scores [B*H, N, M]."""
    from pww_hip import attention as A
    g = torch.Generator().manual_seed(seed)
    q, k = torch.randn(B, N, H * D, generator=g), torch.randn(B, M, H * D, generator=g)
    scores = torch.matmul(O.split_heads(q, H), O.split_heads(k, H).transpose(-1, -2)).reshape(B * H, N, M)
    flat = scores.reshape(B, -1).double()
    monkeypatch.setattr(A.ops, "qk_stats", lambda q_, k_, h: torch.stack([flat.max(1).values, flat.min(1).values, flat.sum(1), (flat ** 2).sum(1)], 1))
    A._warned.discard("materialize")
    return A, A.QKProxy(q, k, H), scores


# every recognised spelling: (call on the proxy, the same call on a tensor, kind name, scope name)
def _spellings():
    head_dims = [(1, 2), (2, 1), (-2, -1), (-1, -2), [1, 2], [-1, -2], (1, -1), (-2, 2)]
    row_dims = [2, -1]
    out = []
    for name, kind in (("amax", "STAT_MAX"), ("amin", "STAT_MIN"), ("mean", "STAT_MEAN"), ("std", "STAT_STD")):
        for scope, dims in (("SCOPE_HEAD", head_dims), ("SCOPE_ROW", row_dims)):
            for dim in dims:
                out.append((lambda t, n=name, d=dim: getattr(t, n)(dim=d, keepdim=True), kind, scope))
                out.append((lambda t, n=name, d=dim: getattr(t, n)(d, keepdim=True), kind, scope))
                if name != "std":
                    out.append((lambda t, n=name, d=dim: getattr(t, n)(d, True), kind, scope))
        out.append((lambda t: t.std(dim=-1, unbiased=True, keepdim=True), "STAT_STD", "SCOPE_ROW") if name == "std" else
                   (lambda t, n=name: getattr(t, n)(keepdim=True, dim=(1, 2)), kind, "SCOPE_HEAD"))
    for scope, dims in (("SCOPE_HEAD", head_dims), ("SCOPE_ROW", row_dims)):
        for dim in dims:
            out.append((lambda t, d=dim: t.abs().amax(dim=d, keepdim=True), "STAT_ABSMAX", scope))
            out.append((lambda t, d=dim: t.abs().amax(d, True), "STAT_ABSMAX", scope))
    return out


def test_recognised_spellings_stay_symbolic_and_materialise_to_the_torch_call(monkeypatch):
    A, p, scores = _proxy(monkeypatch)
    w = torch.rand(6, 5)
    calls = _spellings()
    assert len(calls) > 100
    for call, kind, scope in calls:
        st = call(p)
        assert isinstance(st, A.LazyStat) and st.kind == getattr(A.ops, kind) and st.scope == getattr(A, scope), (kind, scope, st)
        want = call(scores)
        got = st.materialize()
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), (kind, scope)
        assert want.shape == ((4, 1, 1) if scope == "SCOPE_HEAD" else (4, 6, 1))
        # Python factors and ScaledW keep it symbolic
        r = 0.4 * A.ScaledW(w) * 1.5 * (2.0 * st / 4.0)
        assert isinstance(r, A.ScaledW) and r.w is w and r.stat.scope == st.scope and r.stat.kind == st.kind
        sym = A._symbolic_scoped(r)
        assert sym == (st.kind, st.scope, pytest.approx(0.4 * 1.5 * 0.5)) and A._symbolic_scalar(r) is None
        assert torch.allclose(r.materialize(), (0.6 * w) * (want * 0.5), rtol=1e-5, atol=1e-6)
        assert isinstance(-st, A.LazyStat) and (-st).scope == st.scope and torch.equal((-st).materialize(), -want)
    # the image scope is what it was: default scope, same return shape of _symbolic_scalar
    g = A.ScaledW(w) * 2.0 * p.max()
    assert g.stat.scope == A.SCOPE_IMAGE and A._symbolic_scalar(g) == (A.ops.STAT_MAX, 2.0) and A._symbolic_scoped(g) is None
    assert A._symbolic_scalar(A.ScaledW(w) * 3.0) == (A.ops.STAT_NONE, 3.0)


def test_nothing_was_materialised_by_the_symbolic_forms(monkeypatch):
    A, p, scores = _proxy(monkeypatch)
    r_h, r_r = wf_head(A.ScaledW(torch.rand(6, 5)), 3.0, p), wf_row(A.ScaledW(torch.rand(6, 5)), 3.0, p)
    assert p._full is None and "materialize" not in A._warned
    assert A._symbolic_scoped(r_h) == (A.ops.STAT_MAX, A.SCOPE_HEAD, pytest.approx(0.4 * math.log(4.0)))
    assert A._symbolic_scoped(r_r) == (A.ops.STAT_STD, A.SCOPE_ROW, pytest.approx(0.5 * math.log(10.0)))


def test_classify_separates_scopes_and_the_probe_answers_symbolically():
    from pww_hip import attention as A
    w = torch.rand(6, 5)
    probe = lambda: A._ProbeProxy((4, 6, 5), torch.float16, "cpu")      # noqa: E731
    c_head = A.CoeffSlots.classify(wf_head(A.ScaledW(w), 3.0, probe()))
    c_row = A.CoeffSlots.classify(wf_row(A.ScaledW(w), 3.0, probe()))
    c_img = A.CoeffSlots.classify(cases.weight_fn_runner(A.ScaledW(w), torch.tensor(3.0), probe()))
    c_head_std = A.CoeffSlots.classify(A.ScaledW(w) * probe().std(dim=(1, 2), keepdim=True))
    assert c_head[0] == (A.ops.STAT_MAX, A.SCOPE_HEAD) and c_row[0] == (A.ops.STAT_STD, A.SCOPE_ROW) and c_img[0] == A.ops.STAT_MAX
    assert len({c_head[0], c_row[0], c_img[0], c_head_std[0], A.CoeffSlots.NO_BIAS}) == 5
    assert c_head[1] == pytest.approx(0.4 * math.log(4.0)) and c_row[1] == pytest.approx(0.5 * math.log(10.0))
    # a form that is not recognised touches the scores: the probe says so
    with pytest.raises(A._NotSymbolic):
        probe().amax(dim=-1)
    with pytest.raises(A._NotSymbolic):
        probe().std(dim=-1, keepdim=True, correction=0)
    # CoeffSlots.update: a function that changes scope between steps reports "re-capture", as a change of statistic does
    slots = A.CoeffSlots.__new__(A.CoeffSlots)
    slots.sites = [dict(kind=(A.ops.STAT_MAX, A.SCOPE_HEAD), w=w, qk_shape=(4, 6, 5), dtype=torch.float16, device="cpu")]
    stored = []
    orig = A.ops.store_f32
    A.ops.store_f32 = lambda dev, vals: stored.append(list(vals))
    try:
        slots.dev = None
        assert slots.update(wf_head, 2.0) is True and stored[-1] == [pytest.approx(0.4 * math.log(3.0))]
        assert slots.update(wf_row, 2.0) is False
        assert slots.update(lambda w_, s, qk: 0.4 * w_ * qk.amin(dim=(1, 2), keepdim=True), 2.0) is False
        assert slots.update(lambda w_, s, qk: wf_head(w_, s, qk) if s > 1 else wf_row(w_, s, qk), 0.5) is False
    finally:
        A.ops.store_f32 = orig


FALLBACKS = [
    ("keepdim=False", lambda t: t.amax(dim=(1, 2), keepdim=False)[:, None, None]),
    ("keepdim absent", lambda t: t.std(dim=-1)[..., None]),
    ("dim=0", lambda t: t.amax(dim=0, keepdim=True)),
    ("dim=(0, 1)", lambda t: t.mean(dim=(0, 1), keepdim=True)),
    ("unbiased=False", lambda t: t.std(dim=-1, unbiased=False, keepdim=True)),
    ("correction=0", lambda t: t.std(dim=-1, correction=0, keepdim=True)),
    ("correction=1", lambda t: t.std(dim=(1, 2), correction=1, keepdim=True)),
    ("max(dim).values", lambda t: t.max(dim=-1, keepdim=True).values),
    ("min(dim).values", lambda t: t.min(dim=2, keepdim=True).values),
    ("abs().amax without keepdim", lambda t: t.abs().amax(dim=-1)[..., None]),
    ("dim=-2", lambda t: t.amax(dim=-2, keepdim=True)),
]


@pytest.mark.parametrize("name,call", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_everything_else_materialises_and_equals_torch(monkeypatch, name, call):
    A, p, scores = _proxy(monkeypatch)
    w = torch.rand(6, 5)
    with pytest.warns(UserWarning, match="materialising"):
        got = 0.4 * A.ScaledW(w) * math.log(4.0) * call(p)
    want = 0.4 * w * math.log(4.0) * call(scores)
    assert torch.is_tensor(got) and got.shape == want.shape and torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    assert p._full is not None and torch.equal(p._full, scores)


def test_a_second_statistic_factor_goes_through_tensors(monkeypatch):
    A, p, scores = _proxy(monkeypatch)
    w = torch.rand(6, 5)
    flat = scores.reshape(2, -1)
    head, row, img = scores.amax(dim=(1, 2), keepdim=True), scores.std(dim=-1, keepdim=True), flat.max(1).values.reshape(2, 1, 1, 1)
    with pytest.warns(UserWarning, match="materialising"):
        r = (A.ScaledW(w) * p.amax(dim=(1, 2), keepdim=True)) * p.std(dim=-1, keepdim=True)
    assert torch.is_tensor(r) and r.shape == (4, 6, 5) and torch.allclose(r, w * head * row, rtol=1e-5)
    r = (A.ScaledW(w) * 2.0 * p.std(dim=-1, keepdim=True)) * p.max()            # scoped first, a global one second
    assert torch.is_tensor(r) and torch.allclose(r, ((w * 2.0) * row) * img, rtol=1e-5)
    r = (A.ScaledW(w) * p.max()) * p.amax(dim=(1, 2), keepdim=True)             # a global one first
    assert torch.is_tensor(r) and torch.allclose(r, (w * img) * head, rtol=1e-5)
    r = (A.ScaledW(w) * p.amax(dim=(1, 2), keepdim=True)) * torch.tensor(3.0)   # a tensor factor beside a scoped statistic
    assert torch.is_tensor(r) and torch.allclose(r, w * head * 3.0, rtol=1e-5)
    r = A.ScaledW(w) * torch.tensor(3.0) * p.amax(dim=(1, 2), keepdim=True)     # a tensor coefficient first
    assert torch.is_tensor(r) and torch.allclose(r, w * 3.0 * head, rtol=1e-5)
    # tensor arithmetic on a scoped statistic falls back to the real tensor
    assert torch.equal(p.amax(dim=-1, keepdim=True) + 1.0, scores.amax(dim=-1, keepdim=True) + 1.0)
    assert p.mean(dim=(1, 2), keepdim=True).shape == (4, 1, 1)


def test_scope_library_is_built_and_exports_what_its_header_declares(scope_lib_path, built_lib):
    import pww_hip
    from pww_hip import _lib
    header = open(os.path.join(cases.REPO, "include", "pww_hip_scope.h")).read()
    declared = set(re.findall(r"\b(pww_scope_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == set(_lib.SCOPE_EXPORTS), declared ^ set(_lib.SCOPE_EXPORTS)
    nm = subprocess.run(["nm", "-D", "--defined-only", scope_lib_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()[-2] in "TD"}
    assert {s for s in exported if s.startswith("pww")} == declared, exported
    assert not [s for s in exported if not s.startswith("pww") and not s.startswith("__hip") and not s.startswith("_ZN3pww") and s not in ("_init", "_fini")], exported
    assert not [s for s in exported if "set_error" in s or "check_hip" in s]
    assert set(_lib.SCOPE_EXPORTS).isdisjoint(pww_hip.EXPORTS) and set(_lib.SCOPE_EXPORTS).isdisjoint(_lib.LONG_EXPORTS)
    lib = _lib.load_scope()
    assert lib is not None and lib.pww_scope_version() == 100 and lib.pww_scope_last_error() is not None
    assert "build_scope" in open(os.path.join(cases.REPO, "__graft_entry__.py")).read()
    # the product library is what it was: ABI 127, none of the new symbols, at most 6 MiB
    raw = ctypes.CDLL(built_lib)
    assert not any(hasattr(raw, n) for n in _lib.SCOPE_EXPORTS)
    assert pww_hip.load_library().pww_version() == 127 and os.path.getsize(built_lib) <= 6 * 1024 * 1024
    print("libpww_hip_scope.so: %d bytes" % os.path.getsize(scope_lib_path))
    assert os.path.getsize(scope_lib_path) <= 1024 * 1024


class _Attn:
    heads = 2


def test_missing_library_falls_back_and_a_stale_one_raises(monkeypatch, tmp_path, scope_lib_path):
    from pww_hip import _lib, ops, attention as A
    key, w = torch.zeros(1, 77, 2 * 40, dtype=torch.float16), torch.zeros(64, 77)
    route = lambda **kw: A._scoped_route(_Attn(), kw.get("key", key), kw.get("w", w), kw.get("kind", ops.STAT_MAX), A.SCOPE_HEAD, kw.get("rec"), kw.get("lin"))  # noqa: E731
    assert route() is True
    # everything the route does not cover keeps the materialised one
    assert route(key=torch.zeros(1, 154, 80, dtype=torch.float16)) is False and route(key=torch.zeros(1, 129, 80, dtype=torch.float16)) is False
    assert route(key=torch.zeros(1, 128, 80, dtype=torch.float16)) is True
    assert route(rec=object()) is False and route(lin=object()) is False and route(key=key.float()) is False
    assert route(key=torch.zeros(1, 77, 2 * 12, dtype=torch.float16)) is False and route(w=torch.zeros(77, 64).t()) is False
    assert route(key=torch.zeros(1, 1, 80, dtype=torch.float16), kind=ops.STAT_STD) is False
    monkeypatch.setattr(A, "SCOPED_STATS", False)
    assert route() is False
    monkeypatch.setattr(A, "SCOPED_STATS", True)
    # a missing file: the route is simply not taken
    monkeypatch.setitem(_lib._side, "scope", None)
    monkeypatch.setattr(_lib, "SCOPE_LIB_PATH", str(tmp_path / "libpww_hip_scope.so"))
    assert _lib.load_scope() is None and ops.scoped_available() is False and route() is False
    with pytest.raises(_lib.PwwHipError, match="libpww_hip_scope.so not found"):
        ops._scope_lib()
    # a stale one (an older ABI; here: a shared object that reports version 99) raises with the rebuild hint
    src = tmp_path / "stale.c"
    src.write_text("int pww_scope_version(void) { return 99; }\n")
    stale = tmp_path / "libstale.so"
    subprocess.run(["cc", "-shared", "-fPIC", str(src), "-o", str(stale)], check=True)
    monkeypatch.setattr(_lib, "SCOPE_LIB_PATH", str(stale))
    with pytest.raises(_lib.PwwHipError, match="rebuild"):
        _lib.load_scope()
    # a broken one (not a shared object at all) too
    broken = tmp_path / "libbroken.so"
    broken.write_bytes(b"not an ELF file")
    monkeypatch.setattr(_lib, "SCOPE_LIB_PATH", str(broken))
    with pytest.raises(_lib.PwwHipError, match="rebuild"):
        _lib.load_scope()


def _desc(M=77, D=40, N=256, H=8, B=2):
    from pww_hip._lib import AttnDesc
    d = AttnDesc()
    d.dtype, d.B, d.H, d.N, d.M, d.D = 0, B, H, N, M, D
    C = H * D
    d.q_stride[:] = [N * C, D, C]
    d.k_stride[:] = [0, D, C]
    d.v_stride[:] = [0, D, C]
    d.o_stride[:] = [N * C, D, C]
    d.scale = D ** -0.5
    d.bias_stride[:] = [0, 0, M, 1]
    return d


def test_argument_validation_runs_in_front_of_the_first_hip_call(scope_lib_path):
    """Answered without a device (this machine has none: a HIP runtime call would fail with PWW_EHIP instead), so no pointer is touched."""
    from pww_hip import _lib
    from pww_hip._lib import CrossOpts, PWW_EINVAL, PWW_ENOTSUP
    lib = _lib.load_scope()
    P = ctypes.c_void_p(0x10000)       # never dereferenced: validation precedes every launch
    null = ctypes.c_void_p(0)
    err = lambda: lib.pww_scope_last_error().decode()      # noqa: E731
    count = lambda d: lib.pww_scope_head_parts_count(ctypes.byref(d))      # noqa: E731

    def attn(d, q=P, bias=P, opts=None, kind=1, scope=1, parts=P, nparts=None, stats_out=null):
        if nparts is None:
            nparts = count(d) if (d is not None and scope == 1) else 0
        return lib.pww_scope_cross_attn_fwd(q, P, P, P, bias, kind, scope, 1.0, null, ctypes.byref(d) if d is not None else None, parts, nparts,
                                            stats_out, opts, null)

    def parts(d, q=P, out=P, nbytes=1 << 30, kind=1):
        return lib.pww_scope_head_parts(q, P, null, ctypes.byref(d) if d is not None else None, kind, out, nbytes, null)

    d = _desc()
    assert attn(d, q=null) == PWW_EINVAL and "null" in err()
    assert attn(None) == PWW_EINVAL and attn(d, bias=null) == PWW_EINVAL
    assert parts(d, q=null) == PWW_EINVAL and parts(None) == PWW_EINVAL and parts(d, out=null) == PWW_EINVAL
    for M in (129, 154, 256):
        assert attn(_desc(M=M), nparts=2) == PWW_ENOTSUP and "M" in err()
        assert attn(_desc(M=M), scope=2, parts=null) == PWW_ENOTSUP and parts(_desc(M=M)) == PWW_ENOTSUP and count(_desc(M=M)) == 0
    for D in (12, 44, 168):
        assert attn(_desc(D=D), nparts=2) == PWW_ENOTSUP and attn(_desc(D=D), scope=2, parts=null) == PWW_ENOTSUP and parts(_desc(D=D)) == PWW_ENOTSUP
    for scope in (0, 3, -1):
        assert attn(d, scope=scope) == PWW_EINVAL and "scope" in err()
    for kind in (0, 6, 7):
        assert attn(d, kind=kind) == PWW_EINVAL and parts(d, kind=kind) == PWW_EINVAL
    assert attn(_desc(M=1), kind=4, scope=2, parts=null) == PWW_EINVAL and "single score" in err()
    assert attn(_desc(M=1, N=1), kind=4, scope=1) == PWW_EINVAL
    assert attn(d, parts=ctypes.c_void_p(0x10008)) == PWW_EINVAL and "aligned" in err()
    assert parts(d, out=ctypes.c_void_p(0x10008)) == PWW_EINVAL and "aligned" in err()
    assert parts(d, nbytes=2 * 8 * count(d) * 32 - 1) == PWW_EINVAL and "too small" in err()
    assert attn(d, parts=null) == PWW_EINVAL and attn(d, nparts=count(d) + 1) == PWW_EINVAL
    assert attn(d, scope=2, parts=P, nparts=2) == PWW_EINVAL and attn(d, scope=2, parts=null, stats_out=P) == PWW_EINVAL
    short = CrossOpts()
    short.size = 16
    assert attn(d, opts=ctypes.byref(short)) == PWW_EINVAL and "size" in err()
    bad = _desc()
    bad.bias_stride[:] = [0, 0, 1, 256]
    assert attn(bad) == PWW_ENOTSUP and "unit key stride" in err()
    # partials per (image, head): at most 256 for every token count, one per 128 rows up to N = 32768
    for N, want in ((64, 1), (256, 2), (1056, 9), (4096, 32), (9216, 72), (32768, 256), (32769, 129), (1 << 20, 256)):
        assert count(_desc(N=N)) == want, (N, count(_desc(N=N)))


def test_new_unit_has_no_scratch_and_no_spills():
    """hipcc --offload-arch=gfx950 resource usage of every kernel of csrc/pww_scope.hip (tools/check_kernel_invariants.py's remark parser)."""
    sys.path.insert(0, os.path.join(cases.REPO, "tools"))
    import check_kernel_invariants as inv
    import build as pww_build
    flags = [f for u in pww_build.SCOPE_UNITS for f in u[1]] + ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
    rows = inv.resource_usage(os.path.join(inv.CSRC, "pww_scope.hip"), flags)
    kernels = {n: r for n, r in rows.items() if "kernel" in n}
    assert len([n for n in kernels if "scope_attn_kernel" in n]) == 12 and len([n for n in kernels if "scope_head_parts_kernel" in n]) == 12
    for name, r in kernels.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


@pytest.mark.parametrize("shape", ["sd15_n64", "sd15_n256"])
def test_oracle_matches_the_reference_goldens(shape):
    """tests/golden/attn_scoped_<shape>.npz came out of the reference's own inj_forward (tests/scripts/make_scoped_golden.py); the oracle
    reproduces it within the bar tests/test_oracle_golden.py holds the attention goldens to."""
    g = np.load(os.path.join(G, "attn_scoped_%s.npz" % shape))
    case = cases.make_attention_case(shape)
    rows = cases.subsample_rows(case["N"])
    assert np.array_equal(rows, g["rows"])
    for key, wf in (("head", wf_head), ("row", wf_row)):
        y = O.inj_forward(case["attn_cross"], case["hidden"], cases.attention_context(case, "cond", wf))
        ref = g[key]
        assert abs(float(y.abs().double().mean()) - float(g[key + "_absmean"])) <= 1e-6
        err = np.abs(y[0, rows].numpy() - ref).max()
        assert err <= 2e-5 * max(1.0, np.abs(ref).max()), (key, err)
    # the two functions are not the global ones in disguise
    y_img = O.inj_forward(case["attn_cross"], case["hidden"], cases.attention_context(case, "cond", cases.weight_fn_runner))[0, rows].numpy()
    assert np.abs(y_img - g["head"]).max() > 1e-3 and np.abs(g["row"] - g["head"]).max() > 1e-3
