"""CPU stand-ins that several host test modules share (no GPU): fixtures are imported by name into the modules that use them."""
import numpy as np
import pytest
import torch

from oracle import pww_oracle as O


@pytest.fixture
def cpu_masks(monkeypatch):
    """ops.mask_build / mask_build_f32 / gauss_blur as CPU stand-ins built from the oracle's restatements of the same steps."""
    from pww_hip import ops

    def build_f32(masks, cols, ratios=(8, 16, 32, 64)):
        masks = masks.numpy()
        H, W = masks.shape[1:]
        outs = {}
        for r in ratios:
            hr, wr = O.always_round(H / r), O.always_round(W / r)
            out = np.zeros((hr * wr, len(cols)), dtype=np.float32)
            down = {}
            for c, lst in enumerate(cols):
                for reg in lst:
                    if reg not in down:
                        down[reg] = O.bilinear_resize(masks[reg], hr, wr, align_corners=True).reshape(-1)
                    out[:, c] += down[reg]
            outs[r] = torch.from_numpy(out)
        return outs

    def build(rgb, regions, cols, ratios=(8, 16, 32, 64)):
        img = rgb.numpy()
        masks = [(img == np.array(reg[:3], dtype=np.uint8)).all(-1).astype(np.float32) * np.float32(reg[3]) for reg in regions]
        return build_f32(torch.from_numpy(np.stack(masks)), cols, ratios)

    monkeypatch.setattr(ops, "mask_build", build)
    monkeypatch.setattr(ops, "mask_build_f32", build_f32)
    monkeypatch.setattr(ops, "gauss_blur", lambda mask, sigma, ksize=39: torch.from_numpy(O.gaussian_blur(mask.numpy(), sigma, ksize)))
