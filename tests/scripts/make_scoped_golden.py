"""Goldens of the per-head / per-row weight functions: tests/golden/attn_scoped_<shape>.npz.

Runs only where the reference checkout exists (oracle/ref_loader.py AST-loads its `inj_forward` and runs it UNMODIFIED on CPU fp32);
no test imports this script. Only the reference's OUTPUTS are stored: the rows `pww_cases.subsample_rows` picks of `inj_forward` on the
seeded `make_attention_case` inputs, for

    wf_head = 0.4 * w * log(1 + sigma) * qk.amax(dim=(1, 2), keepdim=True)
    wf_row  = 0.5 * w * log(1 + sigma^2) * qk.std(dim=-1, keepdim=True)

    python tests/scripts/make_scoped_golden.py
"""
import math
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pww_cases as cases  # noqa: E402
from oracle import ref_loader  # noqa: E402

SHAPES = ("sd15_n64", "sd15_n256", "sd21_n576")


def wf_head(w, s, qk):
    return 0.4 * w * math.log(1 + s) * qk.amax(dim=(1, 2), keepdim=True)


def wf_row(w, s, qk):
    return 0.5 * w * math.log(1 + s ** 2) * qk.std(dim=-1, keepdim=True)


def main():
    assert ref_loader.available(), "the reference checkout is not here"
    inj = ref_loader.load_reference()["inj_forward"]
    warnings.filterwarnings("ignore")
    for shape in SHAPES:
        case = cases.make_attention_case(shape)
        rows = cases.subsample_rows(case["N"])
        out = {"rows": rows}
        for name, wf in (("head", wf_head), ("row", wf_row)):
            y = inj(case["attn_cross"], case["hidden"], cases.attention_context(case, "cond", wf))
            out[name] = y[0, rows].numpy()
            out[name + "_absmean"] = np.float64(y.abs().double().mean().item())
            print("attn_scoped_%s %s: absmean %.6f" % (shape, name, out[name + "_absmean"]))
        np.savez_compressed(os.path.join(cases.GOLDEN, "attn_scoped_%s.npz" % shape), **out)


if __name__ == "__main__":
    main()
