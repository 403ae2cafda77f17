"""The one loader of the side libraries (pww_hip/_lib.py: SIDE, load_side) without a device, the same cases for each of them: a missing file
follows the table's policy, a stale / short / broken file raises with the rebuild hint, and a real load binds the entry points and the
library's own error slot."""
import ctypes
import subprocess

import pytest

NAMES = ("long", "scope", "linear", "regions")


def _fresh(monkeypatch, name, path):
    """load_side(name) as a process would see it that has not loaded the library, with `path` as the file."""
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, name, None)
    monkeypatch.setattr(_lib, _lib.SIDE[name]["path"], str(path))
    return _lib


def _stub(tmp_path, name, version):
    """a shared object whose only symbol is pww_<name>_version"""
    src = tmp_path / ("stub%d.c" % version)
    src.write_text("int pww_%s_version(void) { return %d; }\n" % (name, version))
    so = tmp_path / ("libstub%d.so" % version)
    subprocess.run(["cc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    return so


def test_the_table_covers_the_four_libraries_and_the_public_names():
    from pww_hip import _lib
    assert tuple(_lib.SIDE) == NAMES
    for name in NAMES:
        spec, up = _lib.SIDE[name], name.upper()
        assert spec["exports"] is getattr(_lib, up + "_EXPORTS") and spec["min_version"] == getattr(_lib, up + "_MIN_VERSION") == 100
        assert spec["path"] == up + "_LIB_PATH" and getattr(_lib, spec["path"]).endswith("libpww_hip_%s.so" % name)
        # every export but the two load_side binds itself has a signature, and nothing else has
        assert set(spec["sigs"]) == set(spec["exports"]) - {"pww_%s_version" % name, "pww_%s_last_error" % name}
        assert callable(getattr(_lib, "load_" + name))
    assert [n for n in NAMES if _lib.SIDE[n]["missing_ok"]] == ["scope"]


@pytest.mark.parametrize("name", NAMES)
def test_a_missing_file_follows_the_policy_of_the_table(monkeypatch, tmp_path, name):
    _lib = _fresh(monkeypatch, name, tmp_path / ("libpww_hip_%s.so" % name))
    load = getattr(_lib, "load_" + name)
    if name == "scope":
        assert load() is None and _lib.load_side(name) is None
        return
    match = "libpww_hip_long.so not found" if name == "long" else "rebuild"
    with pytest.raises(_lib.PwwHipError, match=match):
        load()
    with pytest.raises(_lib.PwwHipError, match="rebuild"):
        _lib.load_side(name)


@pytest.mark.parametrize("name", NAMES)
def test_a_stale_short_or_broken_file_raises_with_the_rebuild_hint(monkeypatch, tmp_path, name):
    # an older ABI: a shared object that reports version 99
    _lib = _fresh(monkeypatch, name, _stub(tmp_path, name, 99))
    with pytest.raises(_lib.PwwHipError, match="rebuild") as e:
        _lib.load_side(name)
    assert "ABI version 99" in str(e.value)
    # the right version, and none of the entry points: the error names what is missing
    _lib = _fresh(monkeypatch, name, _stub(tmp_path, name, 100))
    with pytest.raises(_lib.PwwHipError, match="rebuild") as e:
        getattr(_lib, "load_" + name)()
    assert "lacks" in str(e.value) and all(n in str(e.value) for n in _lib.SIDE[name]["exports"] if not n.endswith("_version"))
    # not a shared object at all
    broken = tmp_path / "libbroken.so"
    broken.write_bytes(b"not an ELF file")
    _lib = _fresh(monkeypatch, name, broken)
    with pytest.raises(_lib.PwwHipError, match="rebuild"):
        _lib.load_side(name)
    # a shared object without the version entry point
    _lib = _fresh(monkeypatch, name, _stub(tmp_path, "other", 101))
    with pytest.raises(_lib.PwwHipError, match="rebuild"):
        _lib.load_side(name)
    assert _lib._side[name] is None          # (nothing of this was cached)


def _null_call(_lib, name, lib):
    """the null-argument call that library's own host test makes: (return code, entry point)"""
    P, null = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)       # never dereferenced: validation precedes every launch
    d = _lib.AttnDesc()
    if name == "long":
        return lib.pww_long_qk_parts(null, P, null, ctypes.byref(d), 1, 0, P, 1 << 30, null), "pww_long_qk_parts"
    if name == "scope":
        return lib.pww_scope_head_parts(null, P, null, ctypes.byref(d), 1, P, 1 << 30, null), "pww_scope_head_parts"
    if name == "linear":
        ld = _lib.LinearDesc(ctypes.sizeof(_lib.LinearDesc), _lib.DTYPE_BF16, 512, 1280, 5120, _lib.LINEAR_BIAS_RESIDUAL, 0, 0, 0, 0, 1)
        return lib.pww_linear_fwd(None, P, P, P, P, ctypes.byref(ld), None, 0, None), "pww_linear_fwd"
    colors = (ctypes.c_uint8 * 24)()
    return lib.pww_regions_masks(None, 512, 512, colors, 5, 0.0, P, None), "pww_regions_masks"


@pytest.mark.parametrize("name", NAMES)
def test_a_real_load_binds_the_entry_points_and_the_library_s_own_error_slot(built_lib, name):
    import build as pww_build
    from pww_hip import _lib
    pww_build.build_side(name)
    lib = _lib.load_side(name)
    assert lib is not None and getattr(_lib, "load_" + name)() is lib and _lib.load_side(name) is lib
    assert getattr(lib, "pww_%s_version" % name)() == 100
    for fn, (argtypes, restype) in _lib.SIDE[name]["sigs"].items():
        assert getattr(lib, fn).argtypes == argtypes and getattr(lib, fn).restype is restype, fn
    product = _lib.load()
    before = product.pww_last_error()
    rc, what = _null_call(_lib, name, lib)
    assert rc == _lib.PWW_EINVAL
    text = getattr(lib, "pww_%s_last_error" % name)().decode()
    assert text and ("null" in text or "required" in text)
    with pytest.raises(_lib.PwwHipError) as e:
        _lib.check(rc, what, lib)
    assert text in str(e.value) and what in str(e.value) and "rc=-22" in str(e.value)
    # the product library's slot is another one
    assert product.pww_last_error() == before and text.encode() != before
