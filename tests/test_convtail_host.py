"""libpww_hip_convtail.so without a device: the build from nothing, the header / export list, the planner's answers to bad descriptors (they
come in front of the first HIP call), and the route of pww_hip/blocks.py declining for each of its reasons on CPU modules."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(built_lib):
    sys.path.insert(0, os.path.join(REPO, "paint-with-words-sd_amd"))
    import build as pww_build
    pww_build.build_convtail()
    from pww_hip import _lib
    return _lib.load_convtail()


def _desc(B=2, H=16, W=16, Cin=1280, C2=2560, Cout=1280, dtype=1, tile_n=0, splitk=0):
    from pww_hip import _lib
    return _lib.ConvTailDesc(ctypes.sizeof(_lib.ConvTailDesc), dtype, B, H, W, Cin, C2, Cout, tile_n, splitk)


def test_builds_from_nothing_into_a_directory_of_its_own(built_lib, tmp_path, monkeypatch):
    """The build row alone makes the library: one translation unit, compiled and linked where no object file or library is yet."""
    import build as pww_build
    out = tmp_path / "libpww_hip_convtail.so"
    monkeypatch.setitem(pww_build.SIDE_PATHS, "convtail", str(out))
    monkeypatch.setattr(pww_build, "HERE", str(tmp_path))            # (the object directory: <HERE>/build/convtail)
    assert pww_build.SIDE_LIBS_CONV["convtail"][0] == "pww_conv_tail.hip" and "convtail" not in pww_build.SIDE_LIBS
    assert pww_build.CONVTAIL_UNITS == [("pww_conv_tail.hip", ["-fvisibility=hidden"], "")]
    assert pww_build.build_side("convtail") == str(out) and out.is_file() and (tmp_path / "build" / "convtail" / "pww_conv_tail.hip.o").is_file()
    assert out.stat().st_size < 512 * 1024
    fresh = ctypes.CDLL(str(out))
    assert fresh.pww_convtail_version() == 100


def test_header_exports_and_the_loader_entry(lib):
    import build as pww_build
    import pww_hip
    from pww_hip import _lib
    header = open(os.path.join(REPO, "include", "pww_hip_convtail.h")).read()
    declared = set(re.findall(r"\b(pww_convtail_\w+)\s*\(", header))
    assert declared == set(_lib.CONVTAIL_EXPORTS), declared ^ set(_lib.CONVTAIL_EXPORTS)
    assert all(hasattr(lib, n) for n in _lib.CONVTAIL_EXPORTS) and lib.pww_convtail_version() == 100 == _lib.CONVTAIL_MIN_VERSION
    assert set(_lib.CONVTAIL_EXPORTS).isdisjoint(pww_hip.EXPORTS)
    assert ctypes.sizeof(_lib.ConvTailDesc) == 40
    # only the declared entry points are visible
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.CONVTAIL_LIB_PATH], capture_output=True, text=True).stdout
    vis = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {v for v in vis if v.startswith("pww_")} == set(_lib.CONVTAIL_EXPORTS)
    assert not [v for v in vis if not v.startswith("pww_convtail_") and v not in ("_init", "_fini")], vis
    spec = _lib.side_spec("convtail")
    assert spec is _lib.SIDE_CONV["convtail"] and spec["missing_ok"] and tuple(_lib.SIDE_CONV) == tuple(pww_build.SIDE_LIBS_CONV)
    assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_convtail_version", "pww_convtail_last_error"}
    assert pww_build.LIB_CONVTAIL == _lib.CONVTAIL_LIB_PATH and _lib.load_side("convtail") is lib
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "for name in pww_build.SIDE_LIBS_CONV" in entry


def test_the_kernel_and_its_measured_table_exist_once():
    """The conv2 + shortcut kernel and TAIL_TUNED are csrc/pww_shortcut_gemm.h and nowhere else: the one-source and the two-source unit
    instantiate that header, neither carries a copy."""
    import glob
    csrc = os.path.join(REPO, "paint-with-words-sd_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) > 20
    for text in ("TAIL_TUNED[]", "__launch_bounds__(CT_THREADS, 2)"):
        holders = [os.path.basename(f) for f in files if text in open(f).read()]
        assert holders == ["pww_shortcut_gemm.h"], (text, holders)
    for unit in ("pww_conv_tail.hip", "pww_concat.hip"):
        assert open(os.path.join(csrc, unit)).read().count('#include "pww_shortcut_gemm.h"') == 1, unit


def test_a_missing_library_is_none_and_the_op_says_so(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "convtail", None)
    monkeypatch.setattr(_lib, "CONVTAIL_LIB_PATH", str(tmp_path / "libpww_hip_convtail.so"))
    assert _lib.load_convtail() is None


def test_workspace_query_follows_the_plan(lib):
    ws = lambda **kw: lib.pww_convtail_workspace_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    assert ws(splitk=1) == 0
    assert ws(splitk=5) == 5 * 4 * 512 * 1280
    n = ws()                                                               # a shape of the measured table: split
    assert n > 0 and n % (4 * 512 * 1280) == 0
    assert ws(B=16, H=64, W=64, Cin=64, C2=64, Cout=64) == 0                # enough tiles: the rule plans no split
    n = ws(B=1, H=5, W=7, Cin=128, C2=192, Cout=192)                        # 3 tiles, 21 slabs: the rule splits, at least 8 slabs per split
    assert n == 2 * 4 * 35 * 192
    assert ws(Cin=64, C2=192, Cout=64, splitk=12) == 12 * 4 * 512 * 64 and ws(Cin=64, C2=192, Cout=64, splitk=13) == 0


def test_the_planner_rejects_a_bad_descriptor_with_a_message(lib):
    from pww_hip import _lib
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    names = ("x", "w", "x2", "w2", "bias", "bias2", "y")

    def call(d, wsp=None, n=0, **ptr):
        args = [ptr.get(k, p) for k in names]
        return lib.pww_convtail_fwd(*args, ctypes.byref(d) if d is not None else None, wsp, n, None)
    err = lib.pww_convtail_last_error
    for bad, word in ((dict(Cin=96), b"multiples of 64"), (dict(C2=2568), b"multiples of 64"), (dict(Cout=1288), b"multiples of 64"), (dict(C2=0), b"C2 0"),
                      (dict(dtype=2), b"dtype 2"), (dict(B=0), b"B 0"), (dict(H=0), b"unsupported"), (dict(B=4096, H=64, W=64), b"2^31"),
                      (dict(Cout=320, tile_n=128), b"tile_n 128"), (dict(tile_n=32), b"tile_n 32"), (dict(splitk=65), b"split 65"),
                      (dict(Cin=64, C2=64, Cout=64, splitk=11), b"exceeds the 10 K-slabs")):
        assert call(_desc(**bad)) == _lib.PWW_ENOTSUP and word in err(), (bad, err())
        assert lib.pww_convtail_workspace_bytes(ctypes.byref(_desc(**bad))) == 0
    short = _desc()
    short.size = 16
    assert call(short) == _lib.PWW_EINVAL and b"older" in err()
    assert call(None) == _lib.PWW_EINVAL and b"missing" in err()
    for k in names:
        assert call(_desc(splitk=1), **{k: None}) == _lib.PWW_EINVAL and b"required" in err(), k
    for k in ("x", "w", "x2", "w2", "y"):
        assert call(_desc(splitk=1), **{k: p + 8}) == _lib.PWW_EINVAL and b"aligned" in err(), k
    assert call(_desc(splitk=1), bias2=p + 4) == _lib.PWW_EINVAL and b"aligned" in err()
    assert call(_desc(splitk=4)) == _lib.PWW_EINVAL and b"workspace" in err()
    assert call(_desc(splitk=4), wsp=p, n=16) == _lib.PWW_EINVAL and b"workspace" in err()
    # a good descriptor with good pointers gets past every check: without a device the first HIP call is what fails
    assert call(_desc(splitk=1)) in (_lib.PWW_EHIP, _lib.PWW_ENOTSUP)


# ---- the route of pww_hip/blocks.py -----------------------------------------------------------------------------------------------------
class _Block:
    pass


def _route_rig(monkeypatch):
    """A ResnetBlock2D's conv2 / conv_shortcut on the CPU with everything the device would answer stubbed to yes: each reason below then
    declines on its own."""
    import torch
    import torch.nn as nn
    from pww_hip import blocks, ops
    monkeypatch.setattr(blocks, "CONV_SHORTCUT", True)
    monkeypatch.setattr(ops, "conv3x3_shortcut_takes", lambda h, w, x, w2: True)
    monkeypatch.setattr(blocks, "_conv3x3_route", lambda conv, x, upsample=False: True)
    monkeypatch.setattr(ops._lib, "load_convtail", lambda: object())
    block = _Block()
    block.conv2 = nn.Conv2d(128, 128, 3, padding=1).to(torch.bfloat16)
    sc = nn.Conv2d(64, 128, 1).to(torch.bfloat16)
    h = torch.zeros(2, 128, 8, 8, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x = torch.zeros(2, 64, 8, 8, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return blocks, block, sc, h, x


def test_the_route_takes_a_plain_shortcut_and_counts_it(monkeypatch):
    import types
    import torch
    blocks, block, sc, h, x = _route_rig(monkeypatch)
    blocks.reset_stats()
    with torch.no_grad():
        assert blocks._conv_shortcut_route(block, sc, h, x, True, 1.0)
        sc.__dict__["_pww_orig_forward"] = sc.forward
        sc.forward = types.MethodType(blocks._conv1x1_forward, sc)          # this plug's own forward on the instance is still "unpatched"
        assert blocks._conv_shortcut_route(block, sc, h, x, True, 1.0)
    st = blocks.stats()
    assert st["conv_shortcut"] == {"fused": 2, "declined": 0} and "conv_shortcut" in blocks._UNRATED and st["hit_rate"] is None


REASONS = ["switch off", "biases not folded", "output_scale_factor", "3 x 3 shortcut", "strided shortcut", "no bias", "foreign forward", "subclass forward",
           "forward hook", "pre-hook", "NCHW input", "input of another dtype", "weight of another dtype", "autograd", "conv2 not 3 x 3", "conv2 strided",
           "shapes the kernel declines", "conv2 off the HIP route", "library missing"]


@pytest.mark.parametrize("reason", REASONS)
def test_the_route_declines(monkeypatch, reason):
    import torch
    import torch.nn as nn
    blocks, block, sc, h, x = _route_rig(monkeypatch)
    from pww_hip import ops
    fold, scale, grad = True, 1.0, False
    if reason == "switch off":
        monkeypatch.setattr(blocks, "CONV_SHORTCUT", False)
    elif reason == "biases not folded":
        fold = False
    elif reason == "output_scale_factor":
        scale = 2.0
    elif reason == "3 x 3 shortcut":
        sc = nn.Conv2d(64, 128, 3, padding=1).to(torch.bfloat16)
    elif reason == "strided shortcut":
        sc = nn.Conv2d(64, 128, 1, stride=2).to(torch.bfloat16)
    elif reason == "no bias":
        sc = nn.Conv2d(64, 128, 1, bias=False).to(torch.bfloat16)
    elif reason == "foreign forward":
        sc.forward = lambda x: x
    elif reason == "subclass forward":
        class Scaled(nn.Conv2d):
            def forward(self, x):
                return 2 * super().forward(x)
        sc = Scaled(64, 128, 1).to(torch.bfloat16)
    elif reason == "forward hook":
        sc.register_forward_hook(lambda m, i, o: o)
    elif reason == "pre-hook":
        sc.register_forward_pre_hook(lambda m, i: i)
    elif reason == "NCHW input":
        x = x.contiguous()
    elif reason == "input of another dtype":
        x = x.float()
    elif reason == "weight of another dtype":
        sc = sc.float()
    elif reason == "autograd":
        grad = True
    elif reason == "conv2 not 3 x 3":
        block.conv2 = nn.Conv2d(128, 128, 1).to(torch.bfloat16)
    elif reason == "conv2 strided":
        block.conv2 = nn.Conv2d(128, 128, 3, stride=2, padding=1).to(torch.bfloat16)
    elif reason == "shapes the kernel declines":
        monkeypatch.setattr(ops, "conv3x3_shortcut_takes", lambda h, w, x, w2: False)
    elif reason == "conv2 off the HIP route":
        monkeypatch.setattr(blocks, "_conv3x3_route", lambda conv, x, upsample=False: False)
    elif reason == "library missing":
        monkeypatch.setattr(ops._lib, "load_convtail", lambda: None)
    blocks.reset_stats()
    with torch.set_grad_enabled(grad):
        assert not blocks._conv_shortcut_route(block, sc, h, x, fold, scale)
    assert blocks.stats()["conv_shortcut"] == {"fused": 0, "declined": 1}


def test_a_cpu_block_keeps_its_own_forward():
    """The whole block on CPU modules: the plug steps aside in front of the route, the result is the module's own."""
    import torch
    from pww_hip import blocks
    from sd_standin import unet as U
    torch.manual_seed(0)
    res = U.ResnetBlock2D(64, 128, 64, 32).eval()
    x, temb = torch.randn(2, 64, 8, 8), torch.randn(2, 64)
    with torch.no_grad():
        ref = res(x, temb)
        blocks.install_blocks(res)
        try:
            blocks.reset_stats()
            got = res(x, temb)
            assert blocks.stats()["conv_shortcut"] == {"fused": 0, "declined": 0}
        finally:
            blocks.uninstall_blocks(res)
    assert torch.equal(got, ref)


def test_takes_declines_on_cpu_tensors():
    import torch
    from pww_hip import ops
    h = torch.zeros(2, 64, 8, 8, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(64, 64, 3, 3, dtype=torch.bfloat16)
    assert not ops.conv3x3_shortcut_takes(h, w, h, torch.zeros(64, 64, 1, 1, dtype=torch.bfloat16))
    with pytest.raises(ops.PwwHipError):
        ops.conv3x3_shortcut(h, w, torch.zeros(64, dtype=torch.bfloat16), h, torch.zeros(64, 64, 1, 1, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.bfloat16))
