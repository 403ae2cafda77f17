"""The case table and probe inputs of tests/attn_route_cases.py, checked without a GPU: the table names every reachable code object of the
general attention launch once, the shapes reach it by a model of the host dispatch, and the probes are strong enough that the GPU test
(test_attn_routes_gpu.py) notices a key that goes missing."""
import pytest
import torch

import attn_route_cases as arc
from attn_route_cases import FOLD, GENERAL, KSPLIT
from gpu_util import TOL

# every (kind, KS, DT, NW, KG, NSUB, HAS_BIAS, ROWSUM_MFMA, RF) the dispatch of csrc/pww_attn_kernel.h can reach in the product library:
# written out, not derived from the table
EXPECTED_ROUTES = [
    # folded d = 8 / 24 / 40
    (FOLD, 3, 2, 2, 1, 2, 0, 1, 1), (FOLD, 3, 2, 4, 1, 2, 0, 1, 1), (FOLD, 3, 2, 8, 1, 2, 0, 1, 1),
    # key-split 4 x 3
    (KSPLIT, 3, 2, 4, 3, 3, 0, 1, 0), (KSPLIT, 3, 2, 4, 3, 3, 0, 0, 0), (KSPLIT, 4, 2, 4, 3, 3, 0, 1, 0), (KSPLIT, 4, 2, 4, 3, 3, 0, 0, 0),
    # key-split 2 x 2
    (KSPLIT, 5, 3, 2, 2, 2, 0, 1, 0), (KSPLIT, 6, 3, 2, 2, 2, 0, 1, 0), (KSPLIT, 6, 3, 2, 2, 2, 0, 0, 0),
    # general, 2 waves
    (GENERAL, 3, 2, 2, 1, 2, 0, 1, 0), (GENERAL, 3, 2, 2, 1, 2, 0, 0, 0), (GENERAL, 4, 2, 2, 1, 1, 0, 1, 0), (GENERAL, 4, 2, 2, 1, 1, 0, 0, 0),
    (GENERAL, 5, 3, 2, 1, 1, 0, 1, 0), (GENERAL, 6, 3, 2, 1, 1, 0, 1, 0), (GENERAL, 6, 3, 2, 1, 1, 0, 0, 0),
    # general, 4 waves, range-free
    (GENERAL, 3, 2, 4, 1, 2, 0, 1, 1), (GENERAL, 3, 2, 4, 1, 2, 0, 0, 1), (GENERAL, 4, 2, 4, 1, 1, 0, 1, 1), (GENERAL, 4, 2, 4, 1, 1, 0, 0, 1),
    (GENERAL, 5, 3, 4, 1, 1, 0, 1, 1), (GENERAL, 6, 3, 4, 1, 1, 0, 1, 1), (GENERAL, 6, 3, 4, 1, 1, 0, 0, 1),
    (GENERAL, 8, 4, 4, 1, 1, 0, 1, 1), (GENERAL, 8, 4, 4, 1, 1, 0, 0, 1), (GENERAL, 10, 5, 4, 1, 1, 0, 1, 1), (GENERAL, 10, 5, 4, 1, 1, 0, 0, 1),
    # general, 8 waves, range-free
    (GENERAL, 3, 2, 8, 1, 2, 0, 1, 1), (GENERAL, 3, 2, 8, 1, 2, 0, 0, 1), (GENERAL, 4, 2, 8, 1, 1, 0, 1, 1), (GENERAL, 4, 2, 8, 1, 1, 0, 0, 1),
    # biased, 2 and 4 waves
    (GENERAL, 3, 2, 2, 1, 2, 1, 0, 0), (GENERAL, 4, 2, 2, 1, 1, 1, 0, 0), (GENERAL, 5, 3, 2, 1, 1, 1, 0, 0), (GENERAL, 6, 3, 2, 1, 1, 1, 0, 0),
    (GENERAL, 3, 2, 4, 1, 2, 1, 0, 0), (GENERAL, 4, 2, 4, 1, 1, 1, 0, 0), (GENERAL, 5, 3, 4, 1, 1, 1, 0, 0), (GENERAL, 6, 3, 4, 1, 1, 1, 0, 0),
    (GENERAL, 8, 4, 4, 1, 1, 1, 0, 0), (GENERAL, 10, 5, 4, 1, 1, 1, 0, 0),
]

# the issue's shapes: head dims per class and row-sum form, key counts per route
HEAD_DIMS = {(3, 2): (16, 32, 48), "fold": (8, 24, 40), (4, 2): (56, 64), (5, 3): (72, 80), (6, 3): (88, 96), (8, 4): (104, 120, 128), (10, 5): (152, 160)}
KEY_COUNTS = {"fold": (200, 577), "general": (200, 577), "ks4x3": (1217, 1024), "ks2x2": (600, 577, 576), "bias": (77, 130)}


def model_route(B, H, N, M, D, bias):
    """The host dispatch (dispatch_nw, dispatch_d, launch_attn, launch_attn_rs) re-stated for the product library with no PWW_DEBUG knob set."""
    rows32 = (N + 31) // 32 * B * H
    wide = (rows32 >= 1024 and N >= 128) or D > 96
    if bias:
        nw = 4 if wide else 2
    elif rows32 >= 2048 and N >= 256 and D <= 64:
        nw = 8
    else:
        nw = 4 if wide else 2
    ks, dt = next(c for lim, c in ((48, (3, 2)), (64, (4, 2)), (80, (5, 3)), (96, (6, 3)), (128, (8, 4)), (160, (10, 5))) if D <= lim)
    assert not (nw == 8 and D > 64) and not (nw == 2 and D > 96)
    rsm = int(D % 32 != 0)
    if not bias:
        if (ks, dt) == (3, 2) and D % 16 == 8:
            return (FOLD, ks, dt, nw, 1, 2, 0, 1, 1)
        if dt <= 2 and nw == 4 and (N + 127) // 128 * B * H <= 256 and M >= 1024:
            return (KSPLIT, ks, dt, 4, 3, 3, 0, rsm, 0)
        if dt == 3 and nw == 2 and (N + 63) // 64 * B * H <= 256 and M >= 512:
            return (KSPLIT, ks, dt, 2, 2, 2, 0, rsm, 0)
    sub_bytes = 64 * (ks * 32 + 16) + 64 * (dt * 64 if dt & 1 else dt * 64 + 64)
    nsub = 2 if 4 * sub_bytes <= 80 * 1024 else 1
    if bias:
        return (GENERAL, ks, dt, nw, 1, nsub, 1, 0, 0)
    return (GENERAL, ks, dt, nw, 1, nsub, 0, rsm, int(nw >= 4))


def test_table_names_every_route_once():
    assert len(EXPECTED_ROUTES) == 42 == len(set(EXPECTED_ROUTES))
    routes = [c.route for c in arc.CASES]
    assert sorted(routes) == sorted(EXPECTED_ROUTES)
    assert len({c.name for c in arc.CASES}) == len(arc.CASES)
    assert arc.SHAPES == {2: (1, 2, 130), 4: (4, 8, 1000), 8: (8, 8, 1000)}


@pytest.mark.parametrize("case", arc.CASES, ids=lambda c: c.name)
def test_shape_takes_its_route_in_the_dispatch_model(case):
    B, H, N = arc.SHAPES[case.nw]
    assert model_route(B, H, N, case.M, case.D, case.bias) == case.route
    assert N != case.M and case.D % 8 == 0
    kind, ks, dt = case.route[:3]
    assert case.D in HEAD_DIMS["fold" if kind == FOLD else (ks, dt)] or (case.bias and case.D == 40)      # (d = 40 with a bias: class (3, 2), not folded)
    group = "bias" if case.bias else "fold" if kind == FOLD else "general" if kind == GENERAL else "ks%dx%d" % case.route[3:5]
    assert case.M in KEY_COUNTS[group]


def test_every_head_dim_and_key_count_is_used():
    dims = {c.D for c in arc.CASES}
    assert dims >= {d for ds in HEAD_DIMS.values() for d in ds}
    for group, counts in KEY_COUNTS.items():
        used = {c.M for c in arc.CASES if (c.bias and group == "bias") or (not c.bias and (
            (group == "fold" and c.route[0] == FOLD) or (group == "general" and c.route[0] == GENERAL)
            or (c.route[0] == KSPLIT and group == "ks%dx%d" % c.route[3:5])))}
        assert used == set(counts), group
    # every probe (row, key) position pair occurs somewhere
    pairs = set()
    for c in arc.CASES:
        N, M = arc.SHAPES[c.nw][2], c.M
        rows, keys = arc.probe_rows(N), arc.probe_keys(M)
        pairs |= {(rows.index(r), keys.index(m)) for _, r, m in arc.probes(c)}
    assert len(pairs) == 24


def test_route_export_without_a_launch(built_lib):
    """pww_debug_last_attn_route on a thread that has launched nothing: PWW_ROUTE_FIELDS fields, kind 0; it writes no more than it is given
    room for and refuses a null buffer."""
    import ctypes
    import threading
    from pww_hip import _lib
    lib = _lib.load()
    seen = {}

    def fresh_thread():
        rec = (ctypes.c_int32 * 12)(*([-7] * 12))
        seen["full"] = (lib.pww_debug_last_attn_route(rec, 12), list(rec))
        rec = (ctypes.c_int32 * 12)(*([-7] * 12))
        seen["short"] = (lib.pww_debug_last_attn_route(rec, 3), list(rec))
        seen["null"] = lib.pww_debug_last_attn_route(None, 9)
    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen["full"] == (9, [0] * 9 + [-7] * 3)
    assert seen["short"] == (9, [0] * 3 + [-7] * 9)
    assert seen["null"] == _lib.PWW_EINVAL
    assert len(arc.ROUTE_FIELDS) == 9


def test_inputs_are_reproducible():
    case = arc.BY_NAME["nw2_ks2x2_d88_m577"]
    a = arc.build(case, torch.bfloat16, "mild")
    arc._base.cache_clear()
    b = arc.build(case, torch.bfloat16, "mild")
    assert all(torch.equal(a[n], b[n]) for n in ("q", "k", "v"))
    assert arc.SEED == 20240


def _probe_rows_reference(case, dtype, variant):
    """Per probe: (share of its key in its row, |change of the row| when that key is dropped, per-row scale s_n), fp64 on the rounded inputs."""
    B, H, N = arc.SHAPES[case.nw]
    inp = arc.build(case, dtype, variant)
    rows = list(arc.probe_rows(N))
    out = []
    by_head = {}
    for j, r, m in arc.probes(case):
        by_head.setdefault(j, []).append((rows.index(r), m))
    for b in range(B):
        O, s, p = arc.reference(inp, b, rows=rows)
        vh = inp["v"][b].double().reshape(case.M, H, case.D).transpose(0, 1)          # [H, M, D]
        for h in range(H):
            for i, m in by_head[b * H + h]:
                pk = p[h, i, m]
                dropped = (O[h, i] - pk * vh[h, m]) / (1.0 - pk)
                out.append((pk.item(), (dropped - O[h, i]).abs().max().item(), s[h, i].item()))
    return out


@pytest.mark.parametrize("dtype", arc.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", arc.CASES, ids=lambda c: c.name)
def test_probes_carry_their_rows(case, dtype):
    """mild: every probe key holds at least 0.15 of its row; strong: at least 0.99; in both, the fp64 reference without that key differs from
    the reference with it by at least 50 per-row bars (TOL s_n): a kernel that loses a probe key cannot pass the GPU test."""
    for variant, share in (("mild", 0.15), ("strong", 0.99)):
        res = _probe_rows_reference(case, dtype, variant)
        assert len(res) == 6 * arc.SHAPES[case.nw][0] * arc.SHAPES[case.nw][1]
        least = min(r[0] for r in res)
        margin = min(r[1] / (TOL[dtype] * r[2]) for r in res)
        print(f"{case.name} {dtype} {variant}: least share of a probe key {least:.3f}, least move of a row without its key {margin:.0f} bars")
        assert least >= share
        assert margin >= 50.0
