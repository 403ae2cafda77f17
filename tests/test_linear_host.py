"""libpww_hip_linear.so without a device: the header / export list, the workspace query and the argument checks of pww_linear_fwd (they run in
front of the first HIP call), and -- under PWW_SLOW=1 -- the static properties of its code objects."""
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
    pww_build.build_linear()
    from pww_hip import _lib
    return _lib.load_linear()


def _desc(M=512, N=1280, K=5120, epilogue=2, dtype=1, xs=0, ys=0, rs=0, tile_n=0, splitk=0):
    from pww_hip import _lib
    return _lib.LinearDesc(ctypes.sizeof(_lib.LinearDesc), dtype, M, N, K, epilogue, xs, ys, rs, tile_n, splitk)


def test_header_and_exports(lib):
    from pww_hip import _lib
    import pww_hip
    header = open(os.path.join(REPO, "include", "pww_hip_linear.h")).read()
    declared = set(re.findall(r"\b(pww_linear_\w+)\s*\(", header))
    assert declared == set(_lib.LINEAR_EXPORTS), declared ^ set(_lib.LINEAR_EXPORTS)
    assert all(hasattr(lib, n) for n in _lib.LINEAR_EXPORTS) and lib.pww_linear_version() == 100
    assert set(_lib.LINEAR_EXPORTS).isdisjoint(pww_hip.EXPORTS)
    assert ctypes.sizeof(_lib.LinearDesc) == 56
    # only the declared entry points are visible
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LINEAR_LIB_PATH], capture_output=True, text=True).stdout
    vis = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {v for v in vis if v.startswith("pww_")} == set(_lib.LINEAR_EXPORTS)


def test_workspace_query_follows_the_plan(lib):
    """No workspace without a split; fp32 partials [split][M][N] with one (N = the GEMM's width, 2 * inner for GEGLU); an explicit split
    overrides the plan; an unsupported descriptor asks for nothing."""
    ws = lambda **kw: lib.pww_linear_workspace_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    assert ws(splitk=1) == 0
    assert ws(splitk=5) == 5 * 4 * 512 * 1280
    assert ws(M=130, N=384, K=320, epilogue=3, splitk=2) == 2 * 4 * 130 * 384
    assert ws(M=65536, N=320, K=320, splitk=0) == 0                      # enough tiles: the rule plans no split
    n = ws(M=100, N=1280, K=2560, splitk=0)                              # 20 tiles: the rule splits, at least 4 slabs per split
    assert n > 0 and n % (4 * 100 * 1280) == 0 and 2 <= n // (4 * 100 * 1280) <= 10
    for bad in (dict(K=5128), dict(N=1288), dict(dtype=2), dict(epilogue=4), dict(N=192, epilogue=3), dict(M=0), dict(splitk=81), dict(tile_n=32),
                dict(N=320, tile_n=128), dict(xs=64), dict(ys=1284), dict(M=1 << 20, K=4096)):
        assert ws(**bad) == 0, bad


def test_argument_checks_run_before_any_hip_call(lib):
    from pww_hip import _lib
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    call = lambda d, x=p, w=p, b=p, r=p, y=p, wsp=None, n=0: lib.pww_linear_fwd(x, w, b, r, y, ctypes.byref(d), wsp, n, None)  # noqa: E731
    assert call(_desc(K=5128)) == _lib.PWW_ENOTSUP and b"multiples of 64" in lib.pww_linear_last_error()
    assert call(_desc(N=192, epilogue=3)) == _lib.PWW_ENOTSUP
    assert call(_desc(dtype=7)) == _lib.PWW_ENOTSUP
    short = _desc()
    short.size = 8
    assert call(short) == _lib.PWW_ENOTSUP and b"older" in lib.pww_linear_last_error()
    assert call(_desc(splitk=1), x=None) == _lib.PWW_EINVAL
    assert call(_desc(splitk=1), b=None) == _lib.PWW_EINVAL and b"bias" in lib.pww_linear_last_error()
    assert call(_desc(splitk=1), r=None) == _lib.PWW_EINVAL
    assert call(_desc(splitk=1), x=p + 2) == _lib.PWW_EINVAL and b"aligned" in lib.pww_linear_last_error()
    assert call(_desc(splitk=4)) == _lib.PWW_EINVAL and b"workspace" in lib.pww_linear_last_error()
    assert call(_desc(splitk=4), wsp=p, n=16) == _lib.PWW_EINVAL


def test_route_table_and_switch():
    sys.path.insert(0, os.path.join(REPO, "paint-with-words-sd_amd"))
    from pww_hip import blocks
    assert "linear" in blocks.stats() and "linear" in blocks._UNRATED
    for M, K, N, epi in blocks.LINEAR_ROUTES:
        assert epi in ("geglu", "residual") and K % 64 == 0 and N % (128 if epi == "geglu" else 64) == 0 and M < 16384


@pytest.mark.slow
def test_linear_kernel_invariants_static():
    """tools/check_kernel_invariants.py --only-linear: no scratch and the register budgets of the linear kernels' code objects."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_kernel_invariants.py"), "--only-linear"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:]
