"""Build libpww_hip.so (gfx950 code objects + C ABI) in-tree with hipcc.

No torch headers are involved: the library is plain HIP behind the C ABI of include/pww_hip.h, and
is loaded from Python with ctypes (pww_hip/_lib.py). hipcc cross-compiles without a GPU.

Fifteen libraries come out of the same sources:
  libpww_hip.so               the product: what the default routes and the documented switches call. `build_lib()`.
  libpww_hip_experiments.so   the same sources with -DPWW_EXPERIMENTS=1 (+ pww_cross_out.hip): the product plus the forms that were built,
                              measured and not made a default (include/pww_hip.h, section "experiments"). Built by the tests / tools that
                              need it (`build_experiments()`, `python build.py --experiments`), never loaded by the product.
  libpww_hip_<name>.so        the side libraries, one per entry of SIDE_LIBS: one translation unit csrc/pww_<name>.hip over the same csrc/
                              headers (its host plumbing is pww_side_host.h), its own entry points pww_<name>_* declared in
                              include/pww_hip_<name>.h and the only visible symbols, loaded by the package on the first call that needs
                              them (pww_hip/_lib.py, `load_side(name)`). `build_side(name)`, or the aliases `build_long()` ...
                              `build_lora()`; __graft_entry__.build() compiles all of them beside the product library.
                                long      the cross-attention launches of prompts longer than 77 tokens (128 < M <= 256 keys)
                                scope     cross-attention whose bias coefficient is a per-head or per-row score statistic (M <= 128 keys)
                                linear    linear layers with a bias / residual / GEGLU epilogue
                                regions   region prompts: the region masks at latent resolution and the per-pixel blend of the noise predictions
                                lora      unmerged LoRA adapters chosen per batch row: the low-rank update behind the attention projections
                              and SIDE_LIBS_CONV, the same kind of row for the side libraries of the convolutions:
                                convtail  conv2 of a ResnetBlock2D with the block's 1 x 1 shortcut as further K-slabs (csrc/pww_conv_tail.hip)
                              and SIDE_LIBS_EXTRA, the open-ended home of every later side library:
                                canvas    canvases larger than the UNet's window: the gather of the windows and the combine of their noise predictions
                                concat    the up blocks without torch.cat: GroupNorm and conv2 + shortcut reading the two halves of the concatenation in place
                                hold      region strength: the strength map of an img2img request, its feather, and the per-step hold of the pixels not yet released
                                convwide  the 160-wide tile of the plain 3 x 3 convolution: csrc/pww_conv.hip compiled for that width alone
                                vae       the AutoencoderKL decoder: the one-head attention of head dim 512 and the tail (norm, SiLU, conv to 3 channels, image)
                                vaeenc    the AutoencoderKL encoder: the head (image -> conv_in), the downsamplers (csrc/pww_conv.hip compiled for stride 2
                                          with the padding on the right and bottom only) and the tail (norm, SiLU, conv to 8 channels, quant_conv, latent)
                                text      the CLIP text encoder: the embedding gather with the first LayerNorm, the causal self-attention of at most
                                          128 tokens with head dim 64, and QuickGELU / GELU in place
A sixteenth joins them, as a row of SIDE_LIBS_EXTRA in front of `text`:
                                control   the residuals of a ControlNet: its 1 x 1 zero convolutions, the conditioning scale and the add into the
                                          UNet's skip tensors as one grouped GEMM
and one more, as a row of SIDE_LIBS_EXTRA in front of `control`:
                                step      one sampler step (Euler, Euler ancestral, DDIM, DPM-Solver++ 2M) as one elementwise launch: the guidance
                                          combine, the scheduler's affine update, the history write and the next UNet input
The large kernel families are instantiated in slices (one translation unit per storage type, the general cross-attention kernel also per
workgroup width) so that the compile runs side by side on the build box's cores.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "pww_hip", "libpww_hip.so")
LIB_EXPERIMENTS = os.path.join(HERE, "pww_hip", "libpww_hip_experiments.so")
# (source, extra defines, object suffix): the instantiation units are compiled once per slice
UNITS = [("pww_api.hip", [], ""), ("pww_attn.hip", [], ""), ("pww_cross.hip", [], ""), ("pww_cross_lean.hip", [], ""), ("pww_reduce.hip", [], ""),
         ("pww_mask.hip", [], ""), ("pww_qproj.hip", [], ""), ("pww_norm.hip", [], ""), ("pww_blocks.hip", [], ""), ("pww_conv.hip", [], ""), ("pww_probs.hip", [], ""),
         ("pww_attn_inst.hip", ["-DPWW_INST_F16"], ".f16"), ("pww_attn_inst.hip", ["-DPWW_INST_BF16"], ".bf16"),
         ("pww_cross_inst.hip", ["-DPWW_INST_F16", "-DPWW_INST_NW=2"], ".f16.nw2"), ("pww_cross_inst.hip", ["-DPWW_INST_F16", "-DPWW_INST_NW=4"], ".f16.nw4"),
         ("pww_cross_inst.hip", ["-DPWW_INST_BF16", "-DPWW_INST_NW=2"], ".bf16.nw2"), ("pww_cross_inst.hip", ["-DPWW_INST_BF16", "-DPWW_INST_NW=4"], ".bf16.nw4")]
EXPERIMENT_UNITS = [("pww_cross_out.hip", [], "")]      # sources only the experiments library has
_ATTN_HEADERS = ["pww_tile.h", "pww_attn_core.h", "pww_cross_tile.h"]
# the side libraries: name -> (translation unit, csrc/ headers besides pww_common.h and pww_side_host.h, what it is). Each is
# pww_hip/libpww_hip_<name>.so behind include/pww_hip_<name>.h, compiled with -fvisibility=hidden: only its pww_<name>_* entry points are
# visible, so a program may link several of them beside the product library.
SIDE_FLAGS = ["-fvisibility=hidden"]
SIDE_LIBS = {
    "long": ("pww_long.hip", _ATTN_HEADERS, "the long-prompt launches"),
    "scope": ("pww_scope.hip", _ATTN_HEADERS, "cross-attention with per-head / per-row score statistics"),
    "linear": ("pww_linear.hip", [], "linear layers with a bias / residual / GEGLU epilogue"),
    "regions": ("pww_regions.hip", [], "region masks and the per-pixel blend of the noise predictions"),
    "lora": ("pww_lora.hip", [], "the per-row low-rank update of unmerged LoRA adapters"),
}
# (a table of its own: SIDE_LIBS is, key for key, the loader's SIDE + SIDE_MORE, and the loader keeps this library in SIDE_CONV)
SIDE_LIBS_CONV = {
    "convtail": ("pww_conv_tail.hip", ["pww_shortcut_gemm.h"], "conv2 of a ResnetBlock2D with the 1 x 1 shortcut as further K-slabs"),
}
# (the open-ended table: SIDE_LIBS and SIDE_LIBS_CONV are closed -- the loader's SIDE + SIDE_MORE and SIDE_CONV, key for key -- and every later
# side library is a row here and in the loader's SIDE_EXTRA, whatever it is for)
SIDE_LIBS_EXTRA = {
    "canvas": ("pww_canvas.hip", [], "canvases larger than the UNet's window: the windows' gather and the combine of their noise predictions"),
    "concat": ("pww_concat.hip", ["pww_shortcut_gemm.h"], "the up blocks without torch.cat: GroupNorm and conv2 + shortcut over the two halves of the concatenation"),
    "hold": ("pww_hold.hip", [], "region strength: the strength map, its feather and the per-step hold of the pixels not yet released"),
    # (pww_conv.hip: the unit IS that file, compiled for the 160-wide tile alone -- the product library has no room for its two code objects)
    "convwide": ("pww_convwide.hip", ["pww_conv.hip"], "the 160-wide tile of the plain 3 x 3 convolution"),
    "vae": ("pww_vae.hip", [], "the AutoencoderKL decoder: one-head attention of head dim 512, and norm + SiLU + conv_out + image in two launches"),
    # (pww_conv.hip again: included with PWW_CONV_DOWN_UNIT, the downsampler's geometry on the 64- and 128-wide tiles)
    "vaeenc": ("pww_vaeenc.hip", ["pww_conv.hip"], "the AutoencoderKL encoder: image -> conv_in, the stride-2 downsamplers, and norm + SiLU + conv_out + quant_conv + latent in two launches"),
    "step": ("pww_step.hip", [], "one sampler step as one launch: guidance combine, the scheduler's affine update, history and the next UNet input"),
    "control": ("pww_control.hip", [], "the residuals of a ControlNet: zero convolutions, conditioning scale and the add into the skips as one grouped GEMM"),
    "text": ("pww_text.hip", [], "the CLIP text encoder: embedding gather + LayerNorm, causal self-attention of head dim 64, QuickGELU / GELU"),
}
ALL_SIDE_LIBS = {**SIDE_LIBS, **SIDE_LIBS_CONV, **SIDE_LIBS_EXTRA}
SOURCES = sorted({u[0] for u in UNITS + EXPERIMENT_UNITS})
HEADERS = ["pww_common.h", "pww_tile.h", "pww_attn_core.h", "pww_attn_kernel.h", "pww_cross_tile.h", "pww_cross_kernel.h", os.path.join(REPO, "include", "pww_hip.h")]
SIDE_PATHS = {n: os.path.join(HERE, "pww_hip", "libpww_hip_%s.so" % n) for n in ALL_SIDE_LIBS}
SIDE_UNITS = {n: [(v[0], SIDE_FLAGS, "")] for n, v in ALL_SIDE_LIBS.items()}     # (as in UNITS)
LIB_LONG, LIB_SCOPE, LIB_LINEAR, LIB_REGIONS, LIB_LORA = (SIDE_PATHS[n] for n in ("long", "scope", "linear", "regions", "lora"))
LONG_UNITS, SCOPE_UNITS, LINEAR_UNITS, REGIONS_UNITS, LORA_UNITS = (SIDE_UNITS[n] for n in ("long", "scope", "linear", "regions", "lora"))
LIB_CONVTAIL, CONVTAIL_UNITS = SIDE_PATHS["convtail"], SIDE_UNITS["convtail"]
LIB_CANVAS, CANVAS_UNITS = SIDE_PATHS["canvas"], SIDE_UNITS["canvas"]
LIB_CONCAT, CONCAT_UNITS = SIDE_PATHS["concat"], SIDE_UNITS["concat"]
LIB_HOLD, HOLD_UNITS = SIDE_PATHS["hold"], SIDE_UNITS["hold"]
LIB_CONVWIDE, CONVWIDE_UNITS = SIDE_PATHS["convwide"], SIDE_UNITS["convwide"]
LIB_VAE, VAE_UNITS = SIDE_PATHS["vae"], SIDE_UNITS["vae"]
LIB_VAEENC, VAEENC_UNITS = SIDE_PATHS["vaeenc"], SIDE_UNITS["vaeenc"]
LIB_TEXT, TEXT_UNITS = SIDE_PATHS["text"], SIDE_UNITS["text"]
LIB_CONTROL, CONTROL_UNITS = SIDE_PATHS["control"], SIDE_UNITS["control"]
LIB_STEP, STEP_UNITS = SIDE_PATHS["step"], SIDE_UNITS["step"]
SIDE_PUBLIC_HEADERS = {"canvas": ["pww_hip_regions.h"]}       # include/ headers a side library's own header includes (besides pww_hip.h)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -amdgpu-kernarg-preload-count=16: the leading SCALAR arguments of a kernel (<= 14 dwords: 16 user SGPRs less the kernarg pointer) are preloaded
# into SGPRs by the dispatcher instead of fetched by the wave's first s_load (gfx950 supports kernarg preload; the compiler keeps a compatibility
# prologue for firmware that does not). Kernels that take one by-value struct are unaffected; the small kernels pass their hot arguments first.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall",
         "-Wno-unused-function", "-mllvm", "-amdgpu-kernarg-preload-count=16"]


# pww_mask.hip, pww_regions.hip, pww_canvas.hip, pww_hold.hip and pww_step.hip restate fp32 formulas that must match a CPU restatement bit for bit: no FMA contraction.
PER_FILE_FLAGS = {"pww_mask.hip": ["-ffp-contract=off"], "pww_regions.hip": ["-ffp-contract=off"], "pww_canvas.hip": ["-ffp-contract=off"],
                  "pww_hold.hip": ["-ffp-contract=off"], "pww_step.hip": ["-ffp-contract=off"]}


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _deps():
    return ([os.path.join(CSRC, s) for s in SOURCES] + [h if os.path.isabs(h) else os.path.join(CSRC, h) for h in HEADERS] + [__file__])


def _build(lib, units, defines, objdir, verbose, jobs=None):
    os.makedirs(objdir, exist_ok=True)
    # longest compiles first (the general cross-attention slices), at most `jobs` at a time
    order = sorted(units, key=lambda u: {"pww_cross_inst.hip": 0, "pww_attn_inst.hip": 1, "pww_cross_lean.hip": 2}.get(u[0], 3))
    # (a shared build box reports far more CPUs than one build may use: MAX_JOBS, or 16)
    jobs = jobs or max(2, min(len(order), os.cpu_count() or 4, int(os.environ.get("MAX_JOBS", 16))))
    pending, running, objs = list(order), [], []
    while pending or running:
        while pending and len(running) < jobs:
            src, defs, suffix = pending.pop(0)
            o = os.path.join(objdir, src + suffix + ".o")
            objs.append(o)
            cmd = [HIPCC] + FLAGS + defines + defs + PER_FILE_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", o]
            if verbose:
                print(" ".join(cmd))
            running.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        cmd, p = running.pop(0)
        out, _ = p.communicate()
        if p.returncode != 0:
            for _, q in running:
                q.kill()
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out))
        if verbose and out.strip():
            print(out)
    # (-s: the host-side symbol table goes -- 100 KB; the exported entry points live in .dynsym, kernel names in the embedded code objects)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-s"] + sorted(objs) + ["-o", lib], check=True)
    return lib


def build_lib(force=False, verbose=False):
    """The product library (what __graft_entry__.build() compiles)."""
    if not force and not _newer(LIB, _deps()):
        return LIB
    return _build(LIB, UNITS, [], os.path.join(HERE, "build"), verbose)


def build_experiments(force=False, verbose=False):
    """libpww_hip_experiments.so: the product + the measured-and-not-default forms (tests and tools only)."""
    if not force and not _newer(LIB_EXPERIMENTS, _deps()):
        return LIB_EXPERIMENTS
    return _build(LIB_EXPERIMENTS, UNITS + EXPERIMENT_UNITS, ["-DPWW_EXPERIMENTS=1"], os.path.join(HERE, "build", "experiments"), verbose)


def build_side(name, force=False, verbose=False):
    """libpww_hip_<name>.so, one of SIDE_LIBS / SIDE_LIBS_CONV / SIDE_LIBS_EXTRA (include/pww_hip_<name>.h)."""
    unit, headers, _ = ALL_SIDE_LIBS[name]
    lib = SIDE_PATHS[name]
    public = ["pww_hip.h", "pww_hip_%s.h" % name] + SIDE_PUBLIC_HEADERS.get(name, [])
    deps = [os.path.join(CSRC, f) for f in [unit, "pww_common.h", "pww_side_host.h"] + headers] + [os.path.join(REPO, "include", h) for h in public] + [__file__]
    if not force and not _newer(lib, deps):
        return lib
    return _build(lib, SIDE_UNITS[name], [], os.path.join(HERE, "build", name), verbose)


def build_long(force=False, verbose=False): return build_side("long", force, verbose)  # noqa: E704
def build_scope(force=False, verbose=False): return build_side("scope", force, verbose)  # noqa: E704
def build_linear(force=False, verbose=False): return build_side("linear", force, verbose)  # noqa: E704
def build_regions(force=False, verbose=False): return build_side("regions", force, verbose)  # noqa: E704
def build_lora(force=False, verbose=False): return build_side("lora", force, verbose)  # noqa: E704
def build_convtail(force=False, verbose=False): return build_side("convtail", force, verbose)  # noqa: E704
def build_canvas(force=False, verbose=False): return build_side("canvas", force, verbose)  # noqa: E704
def build_concat(force=False, verbose=False): return build_side("concat", force, verbose)  # noqa: E704
def build_hold(force=False, verbose=False): return build_side("hold", force, verbose)  # noqa: E704
def build_convwide(force=False, verbose=False): return build_side("convwide", force, verbose)  # noqa: E704
def build_vae(force=False, verbose=False): return build_side("vae", force, verbose)  # noqa: E704
def build_vaeenc(force=False, verbose=False): return build_side("vaeenc", force, verbose)  # noqa: E704
def build_text(force=False, verbose=False): return build_side("text", force, verbose)  # noqa: E704
def build_control(force=False, verbose=False): return build_side("control", force, verbose)  # noqa: E704
def build_step(force=False, verbose=False): return build_side("step", force, verbose)  # noqa: E704


def _build_check(exe, lib, libname, defines, force):
    src = os.path.join(REPO, "tests", "native", "attn_check.cpp")
    if not force and not _newer(exe, [src, lib, os.path.join(REPO, "include", "pww_hip.h")]):
        return exe
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17"] + defines + [src, "-o", exe, "-L" + os.path.dirname(lib), "-l" + libname,
                                                                              "-Wl,-rpath,$ORIGIN/../../paint-with-words-sd_amd/pww_hip"]
    subprocess.run(cmd, check=True)
    return exe


def build_native_check(force=False):
    """tests/native/attn_check: C++ harness that drives the C ABI of the PRODUCT library directly (test infrastructure)."""
    return _build_check(os.path.join(REPO, "tests", "native", "attn_check"), build_lib(), "pww_hip", [], force)


def build_native_check_experiments(force=False):
    """tests/native/attn_check_experiments: the same harness over libpww_hip_experiments.so, with the cases of the moved entry points."""
    return _build_check(os.path.join(REPO, "tests", "native", "attn_check_experiments"), build_experiments(), "pww_hip_experiments", ["-DPWW_EXPERIMENTS=1"], force)


if __name__ == "__main__":
    force = "--force" in sys.argv
    print(build_lib(force=force, verbose=True))
    print(build_native_check(force=force))
    for name in ALL_SIDE_LIBS:
        print(build_side(name, force=force, verbose=True))
    if "--experiments" in sys.argv:
        print(build_experiments(force=force, verbose=True))
        print(build_native_check_experiments(force=force))
