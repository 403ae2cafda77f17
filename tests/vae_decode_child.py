"""Child process of test_vae_decode_gpu.py: the whole decoder under the switches of the environment it was started with (PWW_VAE_ATTN,
PWW_VAE_TAIL), both storage types, the multiple-of-8 latents; the same bars as in the parent (vae_cases.decode_checks). Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "paint-with-words-sd_amd"), REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import vae_cases as C
    from pww_hip import vae as V
    dev = torch.device("cuda:0")
    out = {"attn": V.attn_enabled(), "tail": V.tail_enabled(), "cases": []}
    for dtype in (torch.bfloat16, torch.float16):
        vae = C.make_vae(dtype, dev)
        for shape in C.DECODE_LATENTS:
            st = C.decode_checks(vae, shape, dtype, dev)
            C.assert_native(st, 2, attn=out["attn"], tail=out["tail"])
            out["cases"].append({"dtype": str(dtype), "shape": list(shape), "stats": st})
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
