"""Child process of test_vaeenc_encode_gpu.py: the whole encoder under the switches of the environment it was started with (PWW_VAE_ENC_HEAD,
PWW_VAE_ENC_DOWN, PWW_VAE_ENC_TAIL, PWW_VAE_ATTN), both storage types, the two images; the same bars as in the parent
(vaeenc_cases.encode_checks). Prints one JSON line."""
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
    import vaeenc_cases as C
    from pww_hip import vae as V
    from pww_hip import vae_encode as E
    dev = torch.device("cuda:0")
    out = {"head": E.head_enabled(), "down": E.down_enabled(), "tail": E.tail_enabled(), "attn": V.attn_enabled(), "cases": []}
    for dtype in (torch.bfloat16, torch.float16):
        vae = C.make_vae(dtype, dev)
        for shape in C.ENCODE_IMAGES:
            st = C.encode_checks(vae, shape, dtype, dev)
            C.assert_native(st, 2, attn=out["attn"], head=out["head"], down=out["down"], tail=out["tail"])
            out["cases"].append({"dtype": str(dtype), "shape": list(shape), "stats": st})
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
