"""libpww_hip_concat.so without a device: its rows in the table pair of the open-ended side libraries, the header / export list, the
descriptors, every PWW_ENOTSUP / PWW_EINVAL of its two entry points (they come in front of the first HIP call, with pointers that are never
dereferenced) -- once through ctypes and once from a stand-alone program whose host side is compiled with the address and undefined-
behaviour sanitizers --, and the restated up block of pww_hip/blocks.py on CPU modules, where every call declines to the stock sequence."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "paint-with-words-sd_amd")
EINVAL, ENOTSUP = -22, -95


@pytest.fixture(scope="module")
def lib(built_lib):
    sys.path.insert(0, PKG)
    import build as pww_build
    pww_build.build_concat()
    from pww_hip import _lib
    return _lib.load_concat()


def test_table_rows_header_and_exports(lib):
    import build as pww_build
    import pww_hip
    from pww_hip import _lib
    assert "concat" in pww_build.SIDE_LIBS_EXTRA and tuple(_lib.SIDE_EXTRA) == tuple(pww_build.SIDE_LIBS_EXTRA)
    assert pww_build.SIDE_LIBS_EXTRA["concat"][0] == "pww_concat.hip" and pww_build.CONCAT_UNITS == [("pww_concat.hip", ["-fvisibility=hidden"], "")]
    assert pww_build.LIB_CONCAT == _lib.CONCAT_LIB_PATH and _lib.load_side("concat") is lib
    spec = _lib.side_spec("concat")
    assert spec is _lib.SIDE_EXTRA["concat"] and spec["missing_ok"] and spec["exports"] is _lib.CONCAT_EXPORTS
    assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_concat_version", "pww_concat_last_error"}
    header = open(os.path.join(REPO, "include", "pww_hip_concat.h")).read()
    declared = set(re.findall(r"\b(pww_concat_\w+)\s*\(", header))
    assert declared == set(_lib.CONCAT_EXPORTS), declared ^ set(_lib.CONCAT_EXPORTS)
    assert "#define PWW_CONCAT_VERSION 100" in header
    assert all(hasattr(lib, n) for n in _lib.CONCAT_EXPORTS) and lib.pww_concat_version() == 100 == _lib.CONCAT_MIN_VERSION
    assert set(_lib.CONCAT_EXPORTS).isdisjoint(pww_hip.EXPORTS) and set(_lib.CONCAT_EXPORTS).isdisjoint(_lib.CONVTAIL_EXPORTS)
    for fn, (argtypes, restype) in spec["sigs"].items():
        assert getattr(lib, fn).argtypes == argtypes and getattr(lib, fn).restype is restype, fn
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.CONCAT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    visible = sorted(line.split()[-1] for line in out.splitlines() if " T " in line and not line.split()[-1].startswith(("_init", "_fini")))
    assert visible == sorted(_lib.CONCAT_EXPORTS)            # -fvisibility=hidden: the entry points and nothing else
    source = open(os.path.join(PKG, "csrc", "pww_concat.hip")).read()
    assert source.count('#include "pww_side_host.h"') == 1 and '#define PWW_SIDE_LIB "libpww_hip_concat"' in source
    assert "atomic" not in source.lower() and "pww_norm.hip\"" not in source and "#include \"pww_conv" not in source


def test_the_neighbours_keep_their_exports_and_versions(built_lib):
    """The product library and the convtail library are not touched by this one."""
    import build as pww_build
    import pww_hip
    from pww_hip import _lib
    pww_build.build_convtail()
    assert _lib.load_convtail().pww_convtail_version() == 100
    assert _lib.CONVTAIL_EXPORTS == ("pww_convtail_version", "pww_convtail_last_error", "pww_convtail_workspace_bytes", "pww_convtail_fwd")
    assert not [n for n in pww_hip.EXPORTS if n.startswith("pww_concat")]
    assert [u[0] for u in pww_build.UNITS].count("pww_concat.hip") == 0


def test_descriptor_sizes(lib):
    from pww_hip import _lib
    assert ctypes.sizeof(_lib.ConcatGnDesc) == 40 and ctypes.sizeof(_lib.ConcatTailDesc) == 48
    assert [f[0] for f in _lib.ConcatGnDesc._fields_] == ["size", "dtype", "B", "C1", "C2", "HW", "G", "eps", "act", "_pad"]
    assert [f[0] for f in _lib.ConcatTailDesc._fields_] == ["size", "dtype", "B", "H", "W", "Cin", "C1", "C2", "Cout", "tile_n", "splitk", "_pad"]


def test_a_missing_library_is_none(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "concat", None)
    monkeypatch.setattr(_lib, "CONCAT_LIB_PATH", str(tmp_path / "libpww_hip_concat.so"))
    assert _lib.load_concat() is None


def _gn(B=2, C1=64, C2=32, HW=64, G=8, dtype=1, act=1, size=None):
    from pww_hip import _lib
    return _lib.ConcatGnDesc(ctypes.sizeof(_lib.ConcatGnDesc) if size is None else size, dtype, B, C1, C2, HW, G, 1e-5, act, 0)


def _tail(B=2, H=8, W=8, Cin=64, C1=64, C2=128, Cout=64, dtype=1, tile_n=0, splitk=1, size=None):
    from pww_hip import _lib
    return _lib.ConcatTailDesc(ctypes.sizeof(_lib.ConcatTailDesc) if size is None else size, dtype, B, H, W, Cin, C1, C2, Cout, tile_n, splitk, 0)


def test_the_plans_are_those_of_the_one_source_entry_points(lib, built_lib):
    """Workspace sizes tell the launch form (16 bytes: one launch; otherwise B * nslab * G partials) and the K split: for every shape here
    the two-source library answers what the one-source entry point answers for C1 + C2 channels."""
    from pww_hip import _lib
    product, convtail = _lib.load(), _lib.load_convtail()
    for C1, C2, G in ((64, 32, 8), (64, 64, 32), (8, 24, 4), (64, 32, 16), (1280, 1280, 32), (1288, 1272, 32), (1280, 640, 32), (640, 320, 32), (320, 320, 32)):
        for HW in (4, 35, 40, 64, 256, 576, 1024, 2304, 4096):
            one = _lib.GnDesc(1, _lib.LAYOUT_NHWC, 2, C1 + C2, HW, G, 1e-5, 1, 0, 0)
            assert lib.pww_concat_group_norm_workspace_bytes(ctypes.byref(_gn(C1=C1, C2=C2, HW=HW, G=G))) == product.pww_group_norm_workspace_bytes(ctypes.byref(one)), (C1, C2, G, HW)
    gn_ws = lambda **kw: lib.pww_concat_group_norm_workspace_bytes(ctypes.byref(_gn(**kw)))  # noqa: E731
    assert gn_ws(HW=64) == 16 and gn_ws(HW=2304) == 2 * 14 * 8 * 16 and gn_ws(C1=1280, C2=1280, G=32, HW=576) == 2 * 64 * 32 * 16
    assert gn_ws(HW=35) == 0 and gn_ws(HW=4) == 0                                     # (as the one-source op: HW a multiple of 8)
    # the twelve up-block resnets of SD1.5 at 2 rows, the two down-path shapes of the measured table (640 -> 1280 at 16 x 16, 320 -> 640 at
    # 32 x 32: with them every row of TAIL_TUNED is reached through both entry points), and small shapes: the same split (bytes = split * 4 M Cout)
    for (C1, C2, Cout, side) in ((1280, 1280, 1280, 8), (1280, 1280, 1280, 16), (1280, 640, 1280, 16), (1280, 640, 640, 32), (640, 640, 640, 32), (640, 320, 640, 32),
                                 (640, 320, 320, 64), (320, 320, 320, 64), (320, 320, 1280, 16), (256, 64, 640, 32), (64, 128, 64, 8), (128, 64, 128, 8)):
        for tile_n, splitk in ((0, 0), (64, 0), (0, 5)):
            one = _lib.ConvTailDesc(ctypes.sizeof(_lib.ConvTailDesc), 1, 2, side, side, Cout, C1 + C2, Cout, tile_n, splitk)
            two = _tail(H=side, W=side, Cin=Cout, C1=C1, C2=C2, Cout=Cout, tile_n=tile_n, splitk=splitk)
            assert lib.pww_concat_convtail_workspace_bytes(ctypes.byref(two)) == convtail.pww_convtail_workspace_bytes(ctypes.byref(one)), (C1, C2, Cout, side, tile_n, splitk)


def test_every_refusal_returns_before_a_hip_call(lib):
    from pww_hip import _lib
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    err = lib.pww_concat_last_error
    before = _lib.load().pww_last_error()

    def gn(d, ws=p, n=1 << 20, **ptr):
        args = [ptr.get(k, p) for k in ("x1", "x2", "gamma", "beta", "y")]
        return lib.pww_concat_group_norm_fwd(*args, ctypes.byref(d) if d is not None else None, ws, n, None)
    for bad, word in ((dict(C1=60, C2=36), b"C1 60"), (dict(C2=36, G=4), b"C2 36"), (dict(C1=0, C2=96), b"C1 0"), (dict(HW=35), b"HW 35"), (dict(HW=4), b"HW 4"),
                      (dict(G=7), b"G 7"), (dict(G=48), b"G 48"), (dict(C1=2048, C2=2056), b"4096"), (dict(B=0), b"B 0"), (dict(dtype=2), b"dtype 2"), (dict(act=5), b"act 5")):
        assert gn(_gn(**bad)) == ENOTSUP and b"unsupported" in err() and word in err(), (bad, err())
        assert lib.pww_concat_group_norm_workspace_bytes(ctypes.byref(_gn(**bad))) == 0
    assert gn(_gn(size=8)) == EINVAL and b"older" in err()
    assert gn(None) == EINVAL and b"missing" in err()
    for k in ("x1", "x2", "y"):
        assert gn(_gn(), **{k: None}) == EINVAL and b"required" in err(), k
    assert gn(_gn(), ws=None) == EINVAL and b"required" in err()
    assert gn(_gn(), gamma=None, beta=None) in (_lib.PWW_EHIP, ENOTSUP)                            # (no affine map is a supported call)
    for k in ("x1", "x2", "gamma", "beta", "y"):
        assert gn(_gn(), **{k: p + 8}) == EINVAL and b"aligned" in err(), k
    assert gn(_gn(), ws=p + 8) == EINVAL and b"aligned" in err()
    assert gn(_gn(), n=15) == EINVAL and b"workspace" in err()
    assert gn(_gn(HW=2304), n=2 * 14 * 8 * 16 - 1) == EINVAL and b"workspace" in err()

    names = ("x", "w", "x1", "x2", "wsc", "bias", "bias2", "y")

    def tail(d, ws=None, n=0, **ptr):
        args = [ptr.get(k, p) for k in names]
        return lib.pww_concat_convtail_fwd(*args, ctypes.byref(d) if d is not None else None, ws, n, None)
    for bad, word in ((dict(Cin=96), b"multiples of 64"), (dict(C1=32, C2=96), b"multiples of 64"), (dict(C2=96), b"multiples of 64"), (dict(C1=0), b"C1 0"),
                      (dict(Cout=72), b"multiples of 64"), (dict(dtype=3), b"dtype 3"), (dict(B=0), b"B 0"), (dict(W=0), b"unsupported"),
                      (dict(B=4096, H=64, W=64), b"2^31"), (dict(tile_n=128), b"tile_n 128"), (dict(tile_n=32), b"tile_n 32"), (dict(splitk=65), b"split 65"),
                      (dict(C2=64, splitk=12), b"exceeds the 11 K-slabs")):
        assert tail(_tail(**bad)) == ENOTSUP and word in err(), (bad, err())
        assert lib.pww_concat_convtail_workspace_bytes(ctypes.byref(_tail(**bad))) == 0
    assert tail(_tail(size=12)) == EINVAL and b"older" in err()
    assert tail(None) == EINVAL and b"missing" in err()
    for k in names:
        assert tail(_tail(), **{k: None}) == EINVAL and b"required" in err(), k
    for k in ("x", "w", "x1", "x2", "wsc", "y"):
        assert tail(_tail(), **{k: p + 8}) == EINVAL and b"aligned" in err(), k
    for k in ("bias", "bias2"):
        assert tail(_tail(), **{k: p + 4}) == EINVAL and b"aligned" in err(), k
    assert tail(_tail(splitk=4)) == EINVAL and b"workspace" in err()
    assert tail(_tail(splitk=4), ws=p, n=16) == EINVAL and b"workspace" in err()
    assert tail(_tail(splitk=4), ws=p + 8, n=1 << 30) == EINVAL and b"workspace" in err()
    with pytest.raises(_lib.PwwHipError, match="pww_concat_convtail_fwd failed .rc=-22.*workspace"):
        _lib.check(EINVAL, "pww_concat_convtail_fwd", lib)
    assert _lib.load().pww_last_error() == before            # the product library's error slot is another one
    # good descriptors with good pointers get past every check: without a device the first HIP call is what fails
    assert gn(_gn()) in (_lib.PWW_EHIP, ENOTSUP) and tail(_tail()) in (_lib.PWW_EHIP, ENOTSUP)


def test_the_validation_paths_under_the_sanitizers(tmp_path):
    """tests/native/concat_host_check.cpp + csrc/pww_concat.hip as ONE stand-alone program, host code under -fsanitize=address,undefined
    (nothing is loaded into this interpreter): every refusal again, and the sanitizers must stay silent."""
    import build as pww_build
    exe = str(tmp_path / "concat_host_check")
    cmd = [pww_build.HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "native", "concat_host_check.cpp"),
           os.path.join(PKG, "csrc", "pww_concat.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    # (the HIP runtime's process-lifetime allocations are not this library's: the leak pass is off, every other check is on)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and "concat_host_check OK" in run.stdout, run.stdout + run.stderr
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr


# ---- the restated up block on CPU modules: every resnet call declines, the result is the module's own ------------------------------------
def _up_block(has_attn):
    import torch
    from sd_standin import unet as U
    torch.manual_seed(0)
    return U.UpBlock(128, 64, 64, 64, 2, 2, 96, has_attn, False, 32, False).eval()


@pytest.mark.parametrize("has_attn", [False, True], ids=["plain", "attn"])
def test_a_cpu_up_block_declines_to_the_stock_sequence(has_attn, monkeypatch):
    import torch
    from pww_hip import blocks
    block = _up_block(has_attn)
    g = torch.Generator().manual_seed(1)
    x, skips = torch.randn(2, 64, 8, 8, generator=g), (torch.randn(2, 128, 8, 8, generator=g), torch.randn(2, 64, 8, 8, generator=g))
    temb, ctx = torch.randn(2, 64, generator=g), torch.randn(2, 5, 96, generator=g)
    with torch.no_grad():
        want, rest = block(x, skips, temb, ctx)
        blocks.install_blocks(block)
        try:
            assert getattr(block.__dict__["forward"], "__func__", None) is blocks._up_block_forward
            for on, counted in ((True, {"fused": 0, "declined": 2}), (False, {"fused": 0, "declined": 0})):
                monkeypatch.setattr(blocks, "CONCAT", on)
                blocks.reset_stats()
                got, left = block(x, skips, temb, ctx)
                assert torch.equal(got, want) and left == rest == ()
                assert blocks.stats()["concat"] == counted and "concat" in blocks._UNRATED
            monkeypatch.setattr(blocks, "CONCAT", True)
            blocks.reset_stats()
            got, _ = block(x, skips, temb=temb, ctx=ctx)                   # the same call by keyword
            assert torch.equal(got, want) and blocks.stats()["concat"] == {"fused": 0, "declined": 2}
            # a call the restatement does not know reaches the module's own forward with its arguments untouched
            with pytest.raises(TypeError):
                block(x, skips, temb, ctx, None)
            with pytest.raises(TypeError):
                block(x, skips, temb, ctx=ctx, scale=1.0)
            assert blocks.stats()["concat"] == {"fused": 0, "declined": 2}
            # hooks on the block: its own forward
            handle = block.register_forward_hook(lambda m, i, o: o)
            blocks.reset_stats()
            assert torch.equal(block(x, skips, temb, ctx)[0], want) and blocks.stats()["concat"] == {"fused": 0, "declined": 0}
            handle.remove()
        finally:
            blocks.uninstall_blocks(block)
        assert "forward" not in block.__dict__ and "_pww_orig_forward" not in block.__dict__
        assert torch.equal(block(x, skips, temb, ctx)[0], want)


def test_the_diffusers_signatures_by_class_name():
    """UpBlock2D / CrossAttnUpBlock2D of diffusers 0.10.0, stood in for by classes of those names with that forward: the restatement
    returns what the stock forward returns, and an unknown keyword goes to the module's own forward."""
    import torch
    import torch.nn as nn
    from pww_hip import blocks
    from sd_standin import unet as U

    class _Out:
        def __init__(self, sample):
            self.sample = sample

    class _Attn(nn.Module):
        def forward(self, x, encoder_hidden_states=None):
            return _Out(x + encoder_hidden_states.mean())

    class UpBlock2D(nn.Module):
        def __init__(self):
            super().__init__()
            self.resnets = nn.ModuleList([U.ResnetBlock2D(128, 64, 64, 32), U.ResnetBlock2D(192, 64, 64, 32)])
            self.upsamplers = None
            self.gradient_checkpointing = False

        def forward(self, hidden_states, res_hidden_states_tuple, temb=None, upsample_size=None):
            for resnet in self.resnets:
                hidden_states = resnet(torch.cat([hidden_states, res_hidden_states_tuple[-1]], dim=1), temb)
                res_hidden_states_tuple = res_hidden_states_tuple[:-1]
            return hidden_states

    class CrossAttnUpBlock2D(UpBlock2D):
        def __init__(self):
            super().__init__()
            self.attentions = nn.ModuleList([_Attn(), _Attn()])

        def forward(self, hidden_states, res_hidden_states_tuple, temb=None, encoder_hidden_states=None, upsample_size=None, extra=None):
            for resnet, attn in zip(self.resnets, self.attentions):
                hidden_states = resnet(torch.cat([hidden_states, res_hidden_states_tuple[-1]], dim=1), temb)
                res_hidden_states_tuple = res_hidden_states_tuple[:-1]
                hidden_states = attn(hidden_states, encoder_hidden_states=encoder_hidden_states).sample
            return hidden_states if extra is None else hidden_states + extra

    g = torch.Generator().manual_seed(2)
    x, skips = torch.randn(2, 64, 8, 8, generator=g), (torch.randn(2, 128, 8, 8, generator=g), torch.randn(2, 64, 8, 8, generator=g))
    temb, ctx = torch.randn(2, 64, generator=g), torch.randn(2, 5, 96, generator=g)
    with torch.no_grad():
        for cls, kw in ((UpBlock2D, {}), (CrossAttnUpBlock2D, dict(encoder_hidden_states=ctx))):
            torch.manual_seed(3)
            block = cls().eval()
            want = block(x, skips, temb, **kw)
            blocks.install_blocks(block)
            try:
                blocks.reset_stats()
                assert torch.equal(block(x, skips, temb, **kw), want) and torch.equal(block(hidden_states=x, res_hidden_states_tuple=skips, temb=temb, **kw), want)
                assert blocks.stats()["concat"] == {"fused": 0, "declined": 4}
                if cls is CrossAttnUpBlock2D:
                    assert torch.equal(block(x, skips, temb, extra=1.0, **kw), want + 1.0)                # unknown keyword: the module's own forward
                    assert blocks.stats()["concat"] == {"fused": 0, "declined": 4}
            finally:
                blocks.uninstall_blocks(block)
