"""The recorded latents of the LoRA oracle loops: tests/golden/lora_oracle.npz.

Runs tests/lora_cases.py::oracle_loop -- the fp32 CPU loop in which every row class is evaluated by a deep copy of the UNet with that
class's adapter merged into its weights -- for every entry of lora_cases.RECORDED and prints how far the adapters move the final latent
(the bars tests/test_lora_host.py holds the fixture to). No test imports this script; tests/test_lora_host.py re-runs the loops against the
record.

    python tests/scripts/make_lora_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lora_cases as L  # noqa: E402
from gpu_util import rel_l2  # noqa: E402


def main():
    out = {}
    for name, kw in L.RECORDED.items():
        out[name] = L.oracle_loop(**kw)
        print("ran", name, flush=True)
    print("global vs without            rel-L2 %.4f" % rel_l2(out["global"], out["without"]))
    print("regions vs regions_without   rel-L2 %.4f" % rel_l2(out["regions"], out["regions_without"]))
    print("swapped vs regions           rel-L2 %.4f (and the other way round %.4f)" % (rel_l2(out["swapped"], out["regions"]), rel_l2(out["regions"], out["swapped"])))
    np.savez_compressed(L.GOLDEN, **{k: v.numpy() for k, v in out.items()})
    print("wrote", L.GOLDEN)


if __name__ == "__main__":
    main()
