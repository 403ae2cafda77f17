"""CPU tests of the 3 x 3 convolution route (csrc/pww_conv.hip, pww_hip/ops.py conv3x3, pww_hip/blocks.py): the C ABI's descriptor and
exports, the workspace / plan queries of the library (host code, no GPU), and which modules install_blocks routes and which it leaves alone."""
import ctypes
import os
import re

import torch
import torch.nn as nn

import pww_cases as cases


def test_conv_desc_matches_header():
    from pww_hip import _lib
    header = open(os.path.join(cases.REPO, "include", "pww_hip.h")).read()
    body = header[header.index("typedef struct pww_conv_desc {"):header.index("} pww_conv_desc_t;")]
    names = []
    for decl in re.findall(r"(?:u?int32_t)\s+([^;]+);", re.sub(r"/\*.*?\*/", " ", body, flags=re.S)):
        names += [n.strip() for n in decl.split(",")]
    assert names == [f[0] for f in _lib.ConvDesc._fields_]
    assert ctypes.sizeof(_lib.ConvDesc) == 4 * len(names) == 48
    # declared before the experiments section, exported by the product library
    cut = header.index("= experiments =")
    for name in ("pww_conv3x3_fwd", "pww_conv3x3_workspace_bytes"):
        assert header.index(name) < cut and name in _lib.EXPORTS


def _desc(**kw):
    from pww_hip import _lib
    d = dict(dtype=_lib.DTYPE_BF16, B=2, Hin=16, Win=16, Cin=1280, Cout=1280, stride=1, upsample=0, tile_n=0, splitk=0)
    d.update(kw)
    return _lib.ConvDesc(ctypes.sizeof(_lib.ConvDesc), d["dtype"], d["B"], d["Hin"], d["Win"], d["Cin"], d["Cout"], d["stride"], d["upsample"],
                         d["tile_n"], d["splitk"], 0)


def test_workspace_query_follows_the_plan(built_lib):
    """Split-K only where the tiles alone do not fill the device: none for the batch-8 upsample conv at 32 x 32, fp32 partials [split][M][N]
    at 16 x 16 and 8 x 8; an explicit split overrides the plan; an unsupported descriptor asks for nothing (and the launch refuses it)."""
    import pww_hip
    lib = pww_hip.load_library()
    ws = lambda **kw: lib.pww_conv3x3_workspace_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    assert ws(B=16, Hin=16, Win=16, upsample=1) == 0
    for hw in (16, 8):
        n = ws(Hin=hw, Win=hw)
        M = 2 * hw * hw
        assert n > 0 and n % (4 * M * 1280) == 0 and 2 <= n // (4 * M * 1280) <= 64
    assert ws(Hin=16, Win=16, splitk=1) == 0
    assert ws(Hin=16, Win=16, splitk=5) == 5 * 4 * 512 * 1280
    for bad in (dict(Cin=32), dict(Cin=4), dict(Cout=4), dict(stride=3), dict(upsample=1, stride=2), dict(tile_n=96), dict(dtype=7)):
        assert ws(**bad) == 0, bad
        assert lib.pww_conv3x3_fwd(None, None, None, None, None, ctypes.byref(_desc(**bad)), None, 0, None) != 0
    small = _desc()
    small.size = 8                                     # a descriptor older than the library
    assert lib.pww_conv3x3_workspace_bytes(ctypes.byref(small)) == 0


def test_conv3x3_takes_refuses_cpu_and_odd_widths():
    from pww_hip import ops
    x = torch.zeros(1, 64, 8, 8, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(64, 64, 3, 3, dtype=torch.bfloat16)
    assert not ops.conv3x3_takes(x, w)                 # CPU tensor: no kernel, and no silent CPU path either
    try:
        ops.conv3x3(x, w)
    except ops.PwwHipError:
        pass
    else:
        raise AssertionError("conv3x3 ran on a CPU tensor")


def test_install_blocks_routes_the_3x3_convs():
    """ResnetBlock2D conv1 / conv2 stay unpatched (the block's own restatement calls the kernel, with conv2's bias and the residual in its
    epilogue); Upsample2D is patched by class name and its conv left alone; Downsample2D's conv and other plain 3 x 3 convs get the
    per-instance route; 1 x 1, 3 x 3 with other padding, grouped or dilated convs do not; (n_res, n_gn) is what it was."""
    import pww_hip.blocks as blocks
    from sd_standin import unet as U
    res = U.ResnetBlock2D(64, 128, 32, 32)
    down, up = U.Downsample2D(128), U.Upsample2D(128)
    plain = nn.Conv2d(128, 64, 3, padding=1)
    others = [nn.Conv2d(64, 64, 1), nn.Conv2d(64, 64, 3, padding=0), nn.Conv2d(64, 64, 3, padding=1, groups=2), nn.Conv2d(64, 64, 3, padding=2, dilation=2)]
    model = nn.ModuleList([res, down, up, plain] + others)
    try:
        assert blocks.install_blocks(model) == (1, 0)
        assert "forward" not in res.conv1.__dict__ and "forward" not in res.conv2.__dict__
        assert up.__dict__["forward"].__func__ is blocks._upsample_forward and "forward" not in up.conv.__dict__
        assert down.conv.__dict__["forward"].__func__ is blocks._conv3x3_forward
        assert plain.__dict__["forward"].__func__ is blocks._conv3x3_forward
        assert others[0].__dict__["forward"].__func__ is blocks._conv1x1_forward
        assert all("forward" not in m.__dict__ for m in others[1:])
        # CPU tensors: every route declines to the module's own forward, with the same result
        blocks.reset_stats()
        x = torch.randn(1, 128, 8, 8)
        assert torch.equal(plain(x), nn.Conv2d.forward(plain, x))
        assert torch.equal(down(x), nn.Conv2d.forward(down.conv, x))
        assert torch.equal(up(x), up.conv(torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest")))
        st = blocks.stats()
        assert st["conv3x3"] == {"fused": 0, "declined": 3} and st["hit_rate"] is None       # (not rated)
    finally:
        blocks.uninstall_blocks(model)
    assert all("forward" not in m.__dict__ for m in model.modules())


def test_switch_off_leaves_the_convs_stock(monkeypatch):
    import pww_hip.blocks as blocks
    monkeypatch.setattr(blocks, "CONV3X3", False)
    conv = nn.Conv2d(64, 64, 3, padding=1)
    x = torch.randn(1, 64, 4, 4)
    blocks.reset_stats()
    assert not blocks._conv3x3_route(conv, x)
    assert blocks.stats()["conv3x3"] == {"fused": 0, "declined": 1}
