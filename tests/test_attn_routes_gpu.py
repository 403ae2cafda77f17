"""ops.attention on every code object the general attention launch can reach (tests/attn_route_cases.py: 42 routes x fp16 / bf16), with the
route asserted (pww_debug_last_attn_route) and the probe inputs that make a lost key, a wrong tail mask or a wrong denominator visible.

Per variant (mild, strong, classes, view) of a case:
  1. the launch took the case's route -- a mismatch FAILS (a re-tuned threshold must move the case, not lose the coverage);
  2. every row of the output against the fp64 reference on the same rounded inputs (computed on the GPU, an image at a time);
  3. the project's bar: max|err| <= TOL max|O|;
  4. the per-row bar: |err[n, c]| <= ROW_BAR_U u s_n, s_n = max_c sum_m p_nm |v_mc| from the reference, u = TOL / 4 (one unit in the last place
     of the storage type: 2^-11 fp16, 2^-8 bf16). ROW_BAR_U is the project's 4 u for every route (profiles/attn_route_tests.md lists what
     each route shows);
  5. classes: the class columns of a row sum to 1 within 4 u;
  6. view: no NaN, and bit-identical to the same call on .contiguous() copies;
  7. a second call returns the same bits.
The folded cases (d = 8 / 24 / 40) also assert that no workgroup of `mild` recomputes its rows on the exact path."""
import pytest
import torch

import attn_route_cases as arc
from gpu_util import TOL, last_attn_route, path_counts

pytestmark = pytest.mark.gpu

ROW_BAR_U = 4.0          # per-row bar in units of u s_n, every route


def _run(inp):
    from pww_hip import ops
    return ops.attention(inp["q"], inp["k"], inp["v"], inp["heads"], inp["scale"], bias=inp["bias"], bias_coeff=inp["coeff"])


def _errors(out, inp):
    """(max|err|, max|O|, max err / s_n) over every image, head, row and column, and the fp64 reference's outputs."""
    B, N, C = out.shape
    H = inp["heads"]
    err_max = o_max = row_max = 0.0
    for b in range(B):
        O, s, _ = arc.reference(inp, b)
        err = (out[b].double().reshape(N, H, C // H).transpose(0, 1) - O).abs()
        err_max = max(err_max, err.max().item())
        o_max = max(o_max, O.abs().max().item())
        row_max = max(row_max, (err / s[..., None]).max().item())
    return err_max, o_max, row_max


@pytest.mark.parametrize("dtype", arc.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", arc.CASES, ids=lambda c: c.name)
def test_attention_route(gpu_device, case, dtype):
    B, H, N = arc.SHAPES[case.nw]
    tol, u = TOL[dtype], TOL[dtype] / 4
    failures = []
    for variant in arc.VARIANTS:
        inp = arc.to_device(arc.build(case, dtype, variant), gpu_device)
        call = arc.as_views(inp) if variant == "view" else inp
        if case.route[0] == arc.FOLD and variant == "mild":
            out, paths = path_counts(lambda: _run(call), gpu_device)
            assert sum(paths.values()) == (N + case.nw * 32 - 1) // (case.nw * 32) * B * H and paths["exact"] == 0, paths
        else:
            out = _run(call)
        route = last_attn_route()
        assert route == case.route, "%s: launched %s, the case expects %s (%s)" % (case.name, route, case.route, arc.ROUTE_FIELDS)
        assert torch.equal(out, _run(call)), "%s %s: a second call differs" % (case.name, variant)
        if variant == "view":
            assert not call["k"].is_contiguous() and not call["v"].is_contiguous()
            assert call["q"].untyped_storage().nbytes() == B * (N + arc.PAD_ROWS) * H * case.D * 2       # (NaN rows behind every image's last query row)
            assert not torch.isnan(out).any()
            contiguous = dict(call, q=call["q"].contiguous(), k=call["k"].contiguous(), v=call["v"].contiguous())
            assert torch.equal(out, _run(contiguous)), "%s: strided views and contiguous copies differ" % case.name
        err_max, o_max, row_max = _errors(out, inp)
        print(f"ROUTE {case.name} {str(dtype)[6:]} {variant}: max|err| = {err_max / (tol * o_max):.3f} TOL max|O|, worst err / (u s_n) = {row_max / u:.2f}")
        if not err_max <= tol * o_max:
            failures.append("%s: max|err| %.3e above TOL max|O| = %.3e" % (variant, err_max, tol * o_max))
        if not row_max <= ROW_BAR_U * u:
            failures.append("%s: worst err / (u s_n) = %.2f above %.1f" % (variant, row_max / u, ROW_BAR_U))
        if variant == "classes":
            sums = out.double().reshape(B, N, H, case.D)[..., :arc.NCLS].sum(-1)
            off = (sums - 1.0).abs().max().item()
            print(f"ROUTE {case.name} {str(dtype)[6:]} classes: worst |row sum - 1| = {off / u:.2f} u")
            if not off <= tol:
                failures.append("classes: a row sums to 1 -+ %.2f u" % (off / u))
    assert not failures, "%s %s: %s" % (case.name, dtype, "; ".join(failures))
