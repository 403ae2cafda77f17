"""Prompts longer than 77 tokens, host side (no GPU): the `max_prompt_chunks` keyword, chunking and column mapping on the stand-in
tokenizer, the second library (built, exports, argument validation in front of the first HIP call) and the ISA of its kernels."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess
import sys

import pytest

import pww_cases as cases

PER = 75


def _entry_points():
    pw = importlib.import_module("paint_with_words.paint_with_words")
    inp = importlib.import_module("paint_with_words.paint_with_words_inpaint")
    pipes = importlib.import_module("paint_with_words.pipelines")
    # (the pipeline classes carry the cap as the attribute `max_prompt_chunks`: tests/test_host_logic.py pins the parameter lists of their
    # constructor and __call__ to the reference's, exactly)
    return [pw.paint_with_words, pw.paint_with_words_batch, inp.paint_with_words_inpaint, inp.paint_with_words_inpaint_batch]


def _tokenizer():
    from sd_standin.text import HashTokenizer
    return HashTokenizer()


def _table(tok, phrases):
    from pww_hip import conditioning as C
    ctx = {(i + 1, 0, 0): "%s,1.0" % p for i, p in enumerate(phrases)}
    return C._parse_regions(ctx, tok)


def _prompt(n):
    return " ".join("word%d" % i for i in range(n))


@pytest.fixture(scope="module")
def long_lib_path(built_lib):
    import build as pww_build
    return pww_build.build_long()


def test_keyword_is_last_with_default_one_on_the_function_entry_points():
    for f in _entry_points():
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.name == "max_prompt_chunks" and last.default == 1, (f.__qualname__, last)


def test_more_than_three_chunks_raises_before_anything_else():
    from pww_hip import conditioning as C
    for bad in (0, 4, 7, 2.0, True, None):
        with pytest.raises(ValueError):
            C.check_prompt_chunks(bad)
    eps = _entry_points()
    for f, args in ((eps[0], ()), (eps[1], ({}, None, "", [0])), (eps[2], ()), (eps[3], ({}, None, None, None, "", [0]))):
        with pytest.raises(ValueError, match="max_prompt_chunks"):
            f(*args, max_prompt_chunks=4)
    pipes = importlib.import_module("paint_with_words.pipelines")
    for cls in (pipes.PaintWithWord_StableDiffusionPipeline, pipes.PaintWithWord_StableDiffusionInpaintPipeline):
        assert cls.max_prompt_chunks == 1
        pipe = cls.__new__(cls)
        pipe.max_prompt_chunks = 5          # checked by the call
        with pytest.raises(ValueError, match="max_prompt_chunks"):
            pipe("a prompt", **({"image": 0, "mask_image": 0} if "Inpaint" in cls.__name__ else {}))


def test_short_prompt_with_cap_three_is_the_default_call():
    from pww_hip import conditioning as C
    tok = _tokenizer()
    for n in (0, 1, 20, 75):
        prompt = _prompt(n)
        default = tok([prompt], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")["input_ids"][0].tolist()
        ids, rows = C.chunk_prompt(tok, prompt, 3)
        assert rows == [default] and C.prompt_chunk_count(tok, prompt, 3) == 1
        assert ids == default[1:1 + n]
        table = _table(tok, ["word3 word4", "word19"] if n >= 20 else ["word0"] if n else [])
        assert C.framed_column_lists(table, ids, 1, PER) == C._column_lists(table, default)


def test_column_mapping_on_a_160_token_prompt(capsys):
    from pww_hip import conditioning as C
    tok = _tokenizer()
    prompt = _prompt(160)
    phrases = ["word10 word11 word12", "word74 word75 word76", "word150"]
    table = _table(tok, phrases)
    ids, rows = C.chunk_prompt(tok, prompt, 3)
    assert len(ids) == 160 and len(rows) == 3
    cols = C.framed_column_lists(table, ids, len(rows), PER)
    assert len(cols) == 231
    hit = lambda r: [c for c, lst in enumerate(cols) if r in lst]      # noqa: E731
    assert hit(0) == [11, 12, 13]
    assert hit(1) == [75, 78, 79]           # straddles the first boundary: content 74 | 75, 76
    assert hit(2) == [155]
    assert [C.framed_column(p) for p in (0, 74, 75, 149, 150, 224)] == [1, 75, 78, 152, 155, 229]
    assert "not found" not in capsys.readouterr().out
    # the default cap cuts the prompt at 75 content tokens: phrases past it are warned about, as today
    default = tok([prompt], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")["input_ids"][0].tolist()
    cols1 = C._column_lists(table, default)
    out = capsys.readouterr().out
    assert out.count("not found in text") == 2 and [c for c, lst in enumerate(cols1) if lst] == [11, 12, 13]
    # cap 2: the third chunk's phrase is cut
    ids2, rows2 = C.chunk_prompt(tok, prompt, 2)
    assert len(ids2) == 150 and len(rows2) == 2
    C.framed_column_lists(table, ids2, 2, PER)
    assert capsys.readouterr().out.count("not found in text") == 1
    # nothing depends on where the split falls: the same phrases, prompt shifted by one token
    ids3, rows3 = C.chunk_prompt(tok, "lead " + prompt, 3)
    cols3 = C.framed_column_lists(table, ids3, 3, PER)
    assert [c for c, lst in enumerate(cols3) if 1 in lst] == [78, 79, 80]


def test_framing_and_unconditional_rows():
    from pww_hip import conditioning as C
    from sd_standin.text import BOS, EOS
    tok = _tokenizer()
    ids, rows = C.chunk_prompt(tok, _prompt(160), 3)
    assert [len(r) for r in rows] == [77, 77, 77]
    for j, r in enumerate(rows):
        n = min(PER, 160 - j * PER)
        assert r[0] == BOS and r[1:1 + n] == ids[j * PER:j * PER + n] and all(t == EOS for t in r[1 + n:]) and len(r[1 + n:]) >= 1
    # the unconditional prompt is encoded to the same k, padded with empty chunks
    _, urows = C.chunk_prompt(tok, "", 3, 3)
    assert urows == [[BOS] + [EOS] * 76] * 3
    _, urows = C.chunk_prompt(tok, "blurry, low quality", 2, 2)
    assert len(urows) == 2 and urows[1] == [BOS] + [EOS] * 76 and urows[0][0] == BOS and urows[0][5:] == [EOS] * 72
    # a prompt that needs fewer chunks than the cap gets only the chunks it needs
    assert len(C.chunk_prompt(tok, _prompt(100), 3)[1]) == 2
    # per-image prompts of a batch: padded to the largest count
    pw = importlib.import_module("paint_with_words.paint_with_words")
    assert pw._batch_prompt_chunks(tok, [_prompt(10), _prompt(100), _prompt(160)], 3) == 3
    assert pw._batch_prompt_chunks(tok, [_prompt(10), _prompt(100)], 3) == 2
    assert pw._batch_prompt_chunks(tok, [_prompt(160)], 1) == 1


def test_recorder_uses_the_same_column_mapping():
    from pww_hip import attnmaps, conditioning as C
    tok = _tokenizer()
    ids, rows = C.chunk_prompt(tok, _prompt(160), 3)
    rec = attnmaps.AttentionRecorder.__new__(attnmaps.AttentionRecorder)
    rec.prompts = []
    rec.note_prompt(tok, [t for r in rows for t in r], ids)
    maps = attnmaps.AttentionMaps.__new__(attnmaps.AttentionMaps)      # (columns() reads the tokenizer and the prompts only)
    maps.tokenizer, maps.prompts = rec.tokenizer, list(rec.prompts)
    assert maps.columns("word74 word75 word76") == [75, 78, 79] and maps.columns("word150") == [155]


def test_long_library_is_built_and_exports_what_its_header_declares(long_lib_path, built_lib):
    """build() compiles the second library; it exports exactly the header's declarations; the product library is untouched."""
    import pww_hip
    from pww_hip import _lib
    header = open(os.path.join(cases.REPO, "include", "pww_hip_long.h")).read()
    declared = set(re.findall(r"\b(pww_long_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert declared == set(_lib.LONG_EXPORTS), declared ^ set(_lib.LONG_EXPORTS)
    nm = subprocess.run(["nm", "-D", "--defined-only", long_lib_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()[-2] in "TD"}
    assert {s for s in exported if s.startswith("pww")} == declared, exported
    # (nothing else of the unit is visible: a program may link both libraries)
    assert not [s for s in exported if not s.startswith("pww") and not s.startswith("__hip") and not s.startswith("_ZN3pww") and s not in ("_init", "_fini")], exported
    assert not [s for s in exported if "set_error" in s or "check_hip" in s]
    lib = _lib.load_long()
    assert lib.pww_long_version() == 100 and lib.pww_long_last_error() is not None
    assert "build_long" in open(os.path.join(cases.REPO, "__graft_entry__.py")).read()
    raw = ctypes.CDLL(built_lib)
    assert not any(hasattr(raw, n) for n in _lib.LONG_EXPORTS)
    assert pww_hip.load_library().pww_version() == 127 and os.path.getsize(built_lib) <= 6 * 1024 * 1024
    assert set(pww_hip.EXPORTS).isdisjoint(_lib.LONG_EXPORTS)


def test_missing_long_library_raises(monkeypatch, tmp_path):
    from pww_hip import _lib
    monkeypatch.setitem(_lib._side, "long", None)
    monkeypatch.setattr(_lib, "LONG_LIB_PATH", str(tmp_path / "libpww_hip_long.so"))
    with pytest.raises(_lib.PwwHipError, match="libpww_hip_long.so not found"):
        _lib.load_long()


def _desc(M=231, D=40, N=256, H=8, B=2):
    from pww_hip._lib import AttnDesc
    d = AttnDesc()
    d.dtype, d.B, d.H, d.N, d.M, d.D = 0, B, H, N, M, D
    C = H * D
    d.q_stride[:] = [N * C, D, C]
    d.k_stride[:] = [0, D, C]
    d.v_stride[:] = [0, D, C]
    d.o_stride[:] = [N * C, D, C]
    d.scale = D ** -0.5
    d.bias_stride[:] = [0, 0, M, 1]
    return d


def test_argument_validation_runs_in_front_of_the_first_hip_call(long_lib_path):
    """null pointers, M <= 128 or > 256 -> PWW_ENOTSUP, D % 8, a short opts->size: answered without a device (this machine has none --
    a HIP runtime call would fail with PWW_EHIP instead)."""
    from pww_hip import _lib
    from pww_hip._lib import CrossOpts, ProbsDesc, PWW_EINVAL, PWW_ENOTSUP
    lib = _lib.load_long()
    P = ctypes.c_void_p(0x10000)       # never dereferenced: validation precedes every launch
    null = ctypes.c_void_p(0)
    err = lambda: lib.pww_long_last_error().decode()      # noqa: E731

    def attn(d, q=P, bias=P, opts=None, kind=1, parts=P, nparts=8):
        return lib.pww_long_cross_attn_fwd_parts(q, P, P, P, bias, kind, 1.0, null, ctypes.byref(d) if d is not None else None, parts, nparts, null, opts, null)

    def parts(d, q=P, out=P, nbytes=1 << 30):
        return lib.pww_long_qk_parts(q, P, null, ctypes.byref(d) if d is not None else None, 1, 0, out, nbytes, null)

    pd = ProbsDesc(ctypes.sizeof(ProbsDesc), 0, 0, 1.0)

    def probs(d, q=P, pdesc=pd, opts=None):
        pdesc.out_stride[:] = [256 * 256, 256]
        return lib.pww_long_cross_attn_probs(q, P, null, null, 0, 1.0, 1.0, null, ctypes.byref(d) if d is not None else None, opts, P, ctypes.byref(pdesc), null)

    d = _desc()
    assert attn(d, q=null) == PWW_EINVAL and "null" in err()
    assert attn(None) == PWW_EINVAL and attn(d, bias=null) == PWW_EINVAL
    assert parts(d, q=null) == PWW_EINVAL and parts(None) == PWW_EINVAL and parts(d, out=null) == PWW_EINVAL
    assert probs(d, q=null) == PWW_EINVAL and probs(None) == PWW_EINVAL
    for M in (1, 77, 128, 257, 308):
        for call in (attn, parts, probs):
            assert call(_desc(M=M)) == PWW_ENOTSUP, (call.__name__, M)
            assert "M" in err()
        assert lib.pww_long_qk_parts_count(ctypes.byref(_desc(M=M))) == 0
    for D in (12, 44, 168):
        for call in (attn, parts, probs):
            assert call(_desc(D=D)) == PWW_ENOTSUP, (call.__name__, D)
    short = CrossOpts()
    short.size = 16
    assert attn(d, opts=ctypes.byref(short)) == PWW_EINVAL and "size" in err()
    short.size = 8
    assert probs(d, opts=ctypes.byref(short)) == PWW_EINVAL and "size" in err()
    small = ProbsDesc(8, 0, 0, 1.0)
    assert probs(d, pdesc=small) == PWW_EINVAL
    assert attn(d, kind=1, parts=null) == PWW_EINVAL and parts(d, nbytes=64) == PWW_EINVAL
    # partials per image: at most 256 for every SD layer class at 154 / 231 keys
    for (N, H, D) in ((4096, 8, 40), (1024, 8, 80), (256, 8, 160), (64, 8, 160), (4096, 5, 64), (9216, 16, 64)):
        for M in (154, 231):
            n = lib.pww_long_qk_parts_count(ctypes.byref(_desc(M=M, D=D, N=N, H=H)))
            assert 0 < n <= 256, (N, H, D, M, n)


def test_new_unit_has_no_scratch_and_no_spills():
    """hipcc --offload-arch=gfx950 resource usage of every kernel of csrc/pww_long.hip (tools/check_kernel_invariants.py's remark parser)."""
    sys.path.insert(0, os.path.join(cases.REPO, "tools"))
    import check_kernel_invariants as inv
    import build as pww_build
    flags = [f for u in pww_build.LONG_UNITS for f in u[1]] + ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
    rows = inv.resource_usage(os.path.join(inv.CSRC, "pww_long.hip"), flags)
    kernels = {n: r for n, r in rows.items() if "kernel" in n}
    assert len([n for n in kernels if "cross_long_kernel" in n]) == 12 and any("long_qk_parts_kernel" in n for n in kernels) and any("long_probs_kernel" in n for n in kernels)
    for name, r in kernels.items():
        print("%s: %s VGPRs + %s AGPRs, scratch %s, spills %s / %s" % (name[:70], r["VGPRs"], r["AGPRs"], r["ScratchSize [bytes/lane]"], r["VGPRs Spill"], r["SGPRs Spill"]))
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
