"""CPU tests of the 160-wide tile's plan (host code of csrc/pww_conv.hip, pww_conv_tail.hip, pww_concat.hip; no GPU): tile_n = 160 is
accepted where it divides Cout and refused with the existing error where it does not, the workspace follows the split, Cout = 160 (which
no other width divides) plans the 160-wide tile by itself, and the table-driven defaults ask for what they asked before."""
import ctypes

import pytest


def _conv(tile_n=0, splitk=0, Cout=320, Cin=320, B=2, S=64):
    from pww_hip import _lib
    return _lib.ConvDesc(ctypes.sizeof(_lib.ConvDesc), _lib.DTYPE_BF16, B, S, S, Cin, Cout, 1, 0, tile_n, splitk, 0)


def _tail(tile_n=0, splitk=0, Cout=320, Cin=320, C2=640, B=2, S=64):
    from pww_hip import _lib
    return _lib.ConvTailDesc(ctypes.sizeof(_lib.ConvTailDesc), _lib.DTYPE_BF16, B, S, S, Cin, C2, Cout, tile_n, splitk)


def _cat(tile_n=0, splitk=0, Cout=320, Cin=320, C1=320, C2=320, B=2, S=64):
    from pww_hip import _lib
    return _lib.ConcatTailDesc(ctypes.sizeof(_lib.ConcatTailDesc), _lib.DTYPE_BF16, B, S, S, Cin, C1, C2, Cout, tile_n, splitk, 0)


def _units(built_lib):
    import pww_hip
    from pww_hip import _lib
    main, tail, cat = pww_hip.load_library(), _lib.load_convtail(), _lib.load_concat()
    assert tail is not None and cat is not None
    return [("conv3x3", _conv, main.pww_conv3x3_workspace_bytes, lambda d: main.pww_conv3x3_fwd(None, None, None, None, None, ctypes.byref(d), None, 0, None),
             main.pww_last_error),
            ("convtail", _tail, tail.pww_convtail_workspace_bytes,
             lambda d: tail.pww_convtail_fwd(None, None, None, None, None, None, None, ctypes.byref(d), None, 0, None), tail.pww_convtail_last_error),
            ("concat_convtail", _cat, cat.pww_concat_convtail_workspace_bytes,
             lambda d: cat.pww_concat_convtail_fwd(None, None, None, None, None, None, None, None, ctypes.byref(d), None, 0, None), cat.pww_concat_last_error)]


def test_the_plain_convolution_is_launched_by_exactly_one_library(built_lib):
    """conv3x3's 160-wide code objects live in libpww_hip_convwide.so (csrc/pww_conv.hip compiled for that width alone): both libraries
    plan a descriptor alike (one source), `pww_convwide_takes` says whose it is, and each refuses the other's."""
    import pww_hip
    from pww_hip import _lib
    main, wide = pww_hip.load_library(), _lib.load_convwide()
    assert wide is not None and wide.pww_convwide_version() == 100 == _lib.CONVWIDE_MIN_VERSION
    assert set(_lib.CONVWIDE_EXPORTS).isdisjoint(pww_hip.EXPORTS)
    fwd_main = lambda d: main.pww_conv3x3_fwd(None, None, None, None, None, ctypes.byref(d), None, 0, None)  # noqa: E731
    fwd_wide = lambda d: wide.pww_convwide_fwd(None, None, None, None, None, ctypes.byref(d), None, 0, None)  # noqa: E731
    cases = [(_conv(tile_n=160), 1), (_conv(tile_n=64), 0), (_conv(tile_n=128, Cout=640), 0), (_conv(Cout=160, S=8), 1), (_conv(tile_n=160, Cout=128), 0),
             (_conv(), 1), (_conv(Cin=1280, Cout=1280, S=8), 0)]         # (the last two: the measured table's 320 -> 320 at 64 x 64, and the 8 x 8 level)
    for d, takes in cases:
        assert wide.pww_convwide_takes(ctypes.byref(d)) == takes, (d.Cout, d.tile_n)
        assert main.pww_conv3x3_workspace_bytes(ctypes.byref(d)) == wide.pww_convwide_workspace_bytes(ctypes.byref(d))
    # with every pointer missing the library whose plan it is gets as far as the argument check (EINVAL), the other refuses the plan (ENOTSUP)
    assert fwd_wide(_conv(tile_n=160)) == _lib.PWW_EINVAL and fwd_main(_conv(tile_n=64)) == _lib.PWW_EINVAL
    for d in (_conv(tile_n=160), _conv()):            # (explicit, and the table's choice at tile_n = 0)
        assert fwd_main(d) == _lib.PWW_ENOTSUP and b"libpww_hip_convwide.so (pww_convwide_fwd)" in main.pww_last_error()
    assert fwd_wide(_conv(tile_n=64)) == _lib.PWW_ENOTSUP and b"libpww_hip.so (pww_conv3x3_fwd)" in wide.pww_convwide_last_error()
    assert not _lib.side_spec("convwide")["missing_ok"]      # required: the table plans this tile and the product library cannot launch it


def test_tile_160_is_planned_where_it_divides_cout(built_lib):
    M = 2 * 64 * 64
    for name, desc, ws, fwd, err in _units(built_lib):
        for Cout in (320, 640, 960, 1280, 1920, 2560, 160):
            assert ws(ctypes.byref(desc(tile_n=160, splitk=1, Cout=Cout, S=8))) == 0, (name, Cout)
            assert ws(ctypes.byref(desc(tile_n=160, splitk=3, Cout=Cout, S=8))) == 3 * 4 * 2 * 8 * 8 * Cout, (name, Cout)
        assert ws(ctypes.byref(desc(tile_n=160, splitk=5))) == 5 * 4 * M * 320, name
        # Cout = 160: no other width divides it, the plan takes the 160-wide tile by itself (and a split of its own choice)
        assert ws(ctypes.byref(desc(Cout=160, S=8, splitk=2))) == 2 * 4 * 128 * 160, name
        assert ws(ctypes.byref(desc(Cout=160, S=8, tile_n=64, splitk=2))) == 0 and fwd(desc(Cout=160, S=8, tile_n=64, splitk=2)) != 0, name


def test_tile_160_is_refused_where_it_does_not(built_lib):
    for name, desc, ws, fwd, err in _units(built_lib):
        for Cout in (128, 64, 192, 256):
            d = desc(tile_n=160, Cout=Cout, S=8)
            assert ws(ctypes.byref(d)) == 0 and fwd(d) != 0, (name, Cout)
            assert ("%s: tile_n 160 does not divide Cout %d" % (name, Cout)).encode() in err(), (name, Cout, err())
        d = desc(tile_n=96)
        assert ws(ctypes.byref(d)) == 0 and fwd(d) != 0 and b"tile_n 96 does not divide" in err(), name
        d = desc(Cout=200, S=8)             # neither 64 nor 160 divides it
        assert ws(ctypes.byref(d)) == 0 and fwd(d) != 0 and b"unsupported" in err(), name


@pytest.mark.parametrize("mode", ["plain", "through", "nonsense", None])
def test_partial_stores_switch_moves_no_plan(built_lib, monkeypatch, mode):
    """PWW_PARTIAL_STORES is a store flavour: the workspace a descriptor asks for does not depend on it."""
    want = {}
    monkeypatch.delenv("PWW_PARTIAL_STORES", raising=False)
    for name, desc, ws, fwd, err in _units(built_lib):
        want[name] = [ws(ctypes.byref(desc(tile_n=t, splitk=s))) for t in (0, 64, 160) for s in (0, 2, 5)]
    if mode is not None:
        monkeypatch.setenv("PWW_PARTIAL_STORES", mode)
    for name, desc, ws, fwd, err in _units(built_lib):
        assert [ws(ctypes.byref(desc(tile_n=t, splitk=s))) for t in (0, 64, 160) for s in (0, 2, 5)] == want[name], name
