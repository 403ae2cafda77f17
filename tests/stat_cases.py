"""Case tables, inputs and the fp64 reference of the score-statistic producers: every piece of device code that forms or folds
(max, min, sum, sum of squares) of the raw scores Q K^T. Plain torch, no GPU code: test_score_stats_host.py checks the tables, the inputs
and the dispatch models on the CPU, test_score_stats_gpu.py runs the kernels on them.

  kernel               wrapper                                     scope   forms
  qk_reduce_kernel     ops.qk_stats                                image   2 / 4 waves x head-dim class KS
  qk_parts_kernel      ops.qk_parts                                image   fine / coarse x KS                       (M <= 128)
  long_qk_parts_kernel ops.long_qk_parts                           image   fine / coarse (1 or 2 row blocks a wave) (129 <= M <= 256)
  scope_head_parts_..  ops.scope_head_parts                        head    KS
  qproj_stat_kernel    ops.qproj_stat                              image   tile <NB, TW, CW, KW>, ring of NSETS operand sets, statistic unit
                                                                           (key blocks NKB, compile-time slice count KSC or 0)
  row statistic        ops.attention_scoped(scope=SCOPE_ROW)       row
  fold of partials     stats_out= of ops.attention / attention_scoped

Inputs. All of them are seeded on a CPU generator, made in fp32 and cast to the storage type; the reference is fp64 on the cast tensors.
  neg / pos    dyadic and one-signed: q in {0.75, 1}, k in {-1, -0.75} (pos: k negated). Every score of neg is <= -0.5625 D. All values are exact
               in fp16 and bf16, every product is a multiple of 1/16 and every partial sum stays below 1.5625 * 160 = 250: each score is exact
               in fp32 in whatever order an MFMA adds, so the extremes must equal the reference BIT FOR BIT. A padding zero that reaches max
               (neg) or min (pos) changes the value.
  probe_neg /  neg / pos with the extreme planted at an edge, one position per image: the NEAR probe sets a whole q row to 0.5 and a whole k row
  probe_pos    to -+0.5 (score -+0.25 D in every head: the maximum of neg, the minimum of pos; every other score with one probe vector has
               magnitude >= 0.375 D); the FAR probe (1.25 and -+1.25: -+1.5625 D, the other extreme) sits
               at an edge position that shares neither row nor key with the near probe. Near positions (row, key): image 0 of every case
               (N-1, M-1); the images behind it (0, 0), (N-1, first key of the last 32-key block), (first row of the last 32-row block, M-1)
               in turn, starting at the case's index among its kernel's cases. With K shared between the images the key is planted once (M-1) and the row varies.
  view         the numbers of probe_neg as strided views (as_views()): q = buf[:, :N, :C] of a [B, N + 3, C + 8] buffer, k likewise;
               everything outside the views is NaN, the rows directly behind row N-1 / key M-1 included.
  shifted      not dyadic: q = 0.6 randn + 0.4, k = randn + 0.5 -- the score mean is a few standard deviations from zero. For the sums only.
qproj_stat gets x and W such that Q = x W^T is exact in the storage type: x from the q set, W [C, Cin] with two entries of 0.5 per row at columns
c % Cin and (7 c + 3) % Cin (distinct for even Cin): Q in {0.75, 0.875, 1}, every 64-wide chunk and every contraction wave feeds some channel,
a probe row of x is constant and so is its Q row; the scores are multiples of 1/32 below 250.
"""
import collections
import math

import torch

DTYPES = (torch.float16, torch.bfloat16)
DYADIC = ("neg", "pos", "probe_neg", "probe_pos")
VARIANTS = DYADIC + ("view",)
SEED = 31000
NEAR, FAR = 0.5, 1.25
PAD_ROWS, PAD_COLS = 3, 8
U = 2.0 ** -24                     # unit roundoff of the fp32 accumulation
KS_CLASSES = (3, 4, 5, 6, 8, 10)


def cdiv(a, b):
    return (a + b - 1) // b


def ks_class(D):
    """16-channel slices the kernels of a head dim are instantiated with: D <= 48 -> 3, 64 -> 4, 80 -> 5, 96 -> 6, 128 -> 8, 160 -> 10"""
    return next(ks for lim, ks in ((48, 3), (64, 4), (80, 5), (96, 6), (128, 8), (160, 10)) if D <= lim)


# ---- the host dispatch of every producer, re-stated (checked against the libraries' own counters in test_score_stats_host.py) ----------------

def model_qk_stats(B, H, N, M, D):
    """(waves per workgroup, KS) of qk_reduce_kernel: the attention kernels' wide-groups rule (pww_attn_kernel.h wide_groups)"""
    wide = (cdiv(N, 32) * B * H >= 1024 and N >= 128) or D > 96
    return (4 if wide else 2, ks_class(D))


def model_qk_parts(B, H, N, M, D):
    """((form, KS), partials per image) of qk_parts_kernel (pww_cross_lean.hip): fine = one partial per (head, row block, key block)"""
    nrb, nkb = cdiv(N, 32), cdiv(M, 32)
    coarse = H * nrb * nkb > 256
    return ("coarse" if coarse else "fine", ks_class(D)), (H * cdiv(nrb, 4) if coarse else H * nrb * nkb)


def model_long_qk_parts(B, H, N, M, D):
    """((form, row blocks per wave, KS), partials per image) of long_qk_parts_kernel (pww_long.hip lqk_plan)"""
    nrb, nkb = cdiv(N, 32), cdiv(M, 32)
    if H * nrb * nkb <= 256:
        return ("fine", 1, ks_class(D)), H * nrb * nkb
    rpw = 1
    while rpw < 64 and H * cdiv(nrb, 4 * rpw) > 256:
        rpw *= 2
    return ("coarse", rpw, ks_class(D)), H * cdiv(nrb, 4 * rpw)


def model_scope_head_parts(B, H, N, M, D):
    """((row blocks per wave, KS), partials per (image, head)) of scope_head_parts_kernel (pww_scope.hip)"""
    nrb = cdiv(N, 32)
    rpw = cdiv(nrb, 4 * 256)
    return (rpw, ks_class(D)), cdiv(nrb, 4 * rpw)


QPROJ_TILES = ((5, 4, 1, 1), (5, 2, 1, 2), (5, 1, 1, 4), (10, 2, 2, 1), (10, 1, 2, 2))       # <NB, TW, CW, KW>, in the order qproj_plan tries them
QPROJ_LDS_LIMIT = 160 * 1024 - 1024


def qproj_lds(tile, M):
    nb, tw, cw, kw = tile
    tn, tm = nb * 32, tw * 32
    rowb, red = tn * 2 + 16, (nb // cw) * 16 * 64 * 4
    nred = 0 if kw == 1 else (tw * cw if kw == 2 else 2)
    work = max(kw * (tn + tm) * (64 * 2 + 16), nred * red, tm * rowb)
    return cdiv(M, 32) * 32 * rowb + work + 16 * 8


def model_qproj(B, N, Cin, H, D, M):
    """((NB, TW, CW, KW, NSETS), (NKB, KSC), partials per image) of qproj_stat (pww_qproj.hip qproj_plan and the launch table), None if no
    tile takes the problem. The first tile that gives >= 180 workgroups, else the one with the most; NSETS: the ring of operand sets."""
    C = H * D
    if D % 8 or not 1 <= M <= 128:
        return None
    best, best_wg = None, 0
    for tile in QPROJ_TILES:
        nb, tw, cw, kw = tile
        tn, tm = nb * 32, tw * 32
        if C % tn or tn % D or Cin % (64 * kw) or qproj_lds(tile, M) > QPROJ_LDS_LIMIT:
            continue
        wgs = B * cdiv(N, tm) * (C // tn)
        if wgs >= 180:
            best = tile
            break
        if wgs > best_wg:
            best, best_wg = tile, wgs
    if best is None:
        return None
    nb, tw, cw, kw = best
    ntile, ncg = cdiv(N, tw * 32), C // (nb * 32)
    nsets = {(10, 2): 3, (10, 1): 2, (5, 2): 3, (5, 1): 2}.get((nb, tw)) or (2 if B * ntile * ncg >= 512 else 4)
    nkb = cdiv(M, 32)
    nks = {((h + 1) * D - 1) // 16 - (h * D) // 16 + 1 for h in range(nb * 32 // D)}
    assert len(nks) == 1                    # (every head of a tile spans the same number of 16-channel slices for the head dims in use)
    nks = nks.pop()
    return best + (nsets,), (nkb, nks if nkb == 3 and nks in (3, 4, 5, 10) else 0), ntile * ncg * 4


def qproj_tile_from_count(B, N, Cin, H, D, M, count):
    """The form read back from a partial count alone (the library's pww_qproj_parts): ntile * ncg * 4 fixes (TW, NB) among the candidates
    that take the problem at all (equal counts are equal workgroup counts: qproj_plan keeps the earlier candidate), these fix KW, and the
    ring follows from B * ntile * ncg >= 512. None if no candidate fits."""
    C = H * D
    fits = [t for t in QPROJ_TILES if not (C % (t[0] * 32) or (t[0] * 32) % D or Cin % (64 * t[3]) or qproj_lds(t, M) > QPROJ_LDS_LIMIT)
            and cdiv(N, t[1] * 32) * (C // (t[0] * 32)) * 4 == count]
    if not fits:
        return None
    nb, tw = fits[0][:2]
    wgs = B * count // 4
    return fits[0] + ({(10, 2): 3, (10, 1): 2, (5, 2): 3, (5, 1): 2}.get((nb, tw)) or (2 if wgs >= 512 else 4),)


# ---- case tables ----------------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "kernel name B H N M D Cin shared form")

MODELS = {"qk_stats": model_qk_stats, "qk_parts": model_qk_parts, "long_qk_parts": model_long_qk_parts, "scope_head_parts": model_scope_head_parts}


def _c(kernel, B, H, N, M, D, form, Cin=0, shared=False):
    name = "%s_b%dh%dn%dm%dd%d" % (kernel, B, H, N, M, D) + ("c%d" % Cin if Cin else "") + ("_sharedk" if shared else "")
    return Case(kernel, name, B, H, N, M, D, Cin, shared, form)


CASES = (
    # ---- qk_stats (form: waves, KS). M in {1, 63, 64, 65, 129, 200}, N in {1, 63, 65, 129} and 1000 for the wide rule by rows; D > 96 is always wide
    _c("qk_stats", 2, 2, 1, 63, 8, (2, 3)),
    _c("qk_stats", 2, 2, 63, 1, 40, (2, 3)),
    _c("qk_stats", 2, 2, 65, 64, 64, (2, 4)),
    _c("qk_stats", 2, 2, 129, 65, 80, (2, 5)),
    _c("qk_stats", 2, 2, 63, 129, 96, (2, 6)),
    _c("qk_stats", 1, 2, 65, 200, 128, (4, 8)),
    _c("qk_stats", 2, 2, 129, 200, 160, (4, 10), shared=True),
    _c("qk_stats", 4, 8, 1000, 65, 8, (4, 3)),
    _c("qk_stats", 4, 8, 1000, 129, 64, (4, 4), shared=True),
    _c("qk_stats", 4, 8, 1000, 63, 80, (4, 5)),
    _c("qk_stats", 4, 8, 1000, 200, 96, (4, 6)),
    # ---- qk_parts (form: fine / coarse, KS). fine: M in {1, 32, 33, 64, 77, 96, 97, 128}, N in {1, 31, 33, 70}
    _c("qk_parts", 2, 2, 1, 1, 8, ("fine", 3)),
    _c("qk_parts", 2, 2, 31, 32, 40, ("fine", 3)),
    _c("qk_parts", 2, 3, 33, 33, 64, ("fine", 4)),
    _c("qk_parts", 2, 2, 70, 64, 80, ("fine", 5), shared=True),
    _c("qk_parts", 1, 2, 33, 77, 96, ("fine", 6)),
    _c("qk_parts", 2, 2, 70, 96, 128, ("fine", 8)),
    _c("qk_parts", 1, 2, 31, 97, 160, ("fine", 10)),
    _c("qk_parts", 2, 2, 70, 128, 40, ("fine", 3)),
    # coarse: 35 row blocks -- the last workgroup of a head has three live waves and one that owns only padding
    _c("qk_parts", 2, 8, 1100, 77, 40, ("coarse", 3), shared=True),
    _c("qk_parts", 1, 8, 1100, 128, 64, ("coarse", 4)),
    _c("qk_parts", 1, 8, 1100, 77, 80, ("coarse", 5)),
    _c("qk_parts", 1, 8, 1100, 128, 96, ("coarse", 6)),
    _c("qk_parts", 1, 8, 1100, 33, 128, ("coarse", 8)),
    _c("qk_parts", 2, 8, 1100, 128, 160, ("coarse", 10)),
    # ---- long_qk_parts (form: fine / coarse, row blocks per wave, KS). M in {129, 160, 161, 231, 256}
    _c("long_qk_parts", 2, 2, 33, 129, 40, ("fine", 1, 3)),
    _c("long_qk_parts", 2, 2, 70, 160, 64, ("fine", 1, 4), shared=True),
    _c("long_qk_parts", 1, 2, 33, 161, 80, ("fine", 1, 5)),
    _c("long_qk_parts", 2, 3, 70, 231, 96, ("fine", 1, 6)),
    _c("long_qk_parts", 1, 2, 70, 256, 160, ("fine", 1, 10)),
    _c("long_qk_parts", 2, 16, 70, 256, 8, ("coarse", 1, 3)),              # (3 row blocks: the fourth wave owns none)
    _c("long_qk_parts", 1, 20, 33, 231, 40, ("coarse", 1, 3)),
    _c("long_qk_parts", 1, 8, 4200, 129, 128, ("coarse", 2, 8)),           # (132 row blocks, 8 per workgroup: the last one has half of them)
    # ---- scope_head_parts (form: row blocks per wave, KS). N in {1, 33, 128, 129, 1056}, M in {5, 32, 77, 97, 128}
    _c("scope_head_parts", 2, 2, 1, 5, 8, (1, 3)),
    _c("scope_head_parts", 2, 3, 33, 32, 64, (1, 4)),
    _c("scope_head_parts", 2, 2, 128, 77, 40, (1, 3)),
    _c("scope_head_parts", 2, 2, 129, 97, 160, (1, 10), shared=True),
    _c("scope_head_parts", 1, 2, 1056, 128, 40, (1, 3)),
    _c("scope_head_parts", 2, 2, 33, 77, 8, (1, 3)),
    # ---- qproj_stat (form: (NB, TW, CW, KW, NSETS), (NKB, KSC)). Heads of 160 channels never reach a 320-channel tile (a 160-channel tile
    # always has at least as many workgroups) and <10, 1, 2, 2> does not fit the LDS with three key blocks (M > 64): see profiles/score_stats_tests.md
    _c("qproj_stat", 1, 32, 2900, 77, 40, ((5, 4, 1, 1, 4), (3, 3)), Cin=64),        # ring of 4 over a contraction of ONE chunk
    _c("qproj_stat", 1, 32, 2900, 33, 40, ((5, 4, 1, 1, 4), (2, 0)), Cin=320),
    _c("qproj_stat", 1, 32, 8100, 64, 40, ((5, 4, 1, 1, 2), (2, 0)), Cin=64),
    _c("qproj_stat", 2, 8, 70, 33, 40, ((5, 2, 1, 2, 3), (2, 0)), Cin=128),          # ring of 3 over one chunk per contraction wave
    _c("qproj_stat", 2, 8, 70, 77, 40, ((5, 2, 1, 2, 3), (3, 3)), Cin=128, shared=True),
    _c("qproj_stat", 2, 8, 70, 96, 40, ((5, 2, 1, 2, 3), (3, 3)), Cin=128),          # whole key blocks: neg[] all zero
    _c("qproj_stat", 2, 2, 70, 77, 160, ((5, 2, 1, 2, 3), (3, 10)), Cin=128),
    _c("qproj_stat", 2, 5, 70, 77, 32, ((5, 2, 1, 2, 3), (3, 0)), Cin=128),          # run-time slice loop with 3 key blocks
    _c("qproj_stat", 2, 20, 70, 77, 8, ((5, 2, 1, 2, 3), (3, 0)), Cin=128),
    _c("qproj_stat", 2, 8, 70, 77, 40, ((5, 1, 1, 4, 2), (3, 3)), Cin=256),
    _c("qproj_stat", 2, 8, 70, 128, 40, ((5, 1, 1, 4, 2), (4, 0)), Cin=256),
    _c("qproj_stat", 2, 4, 70, 77, 80, ((5, 1, 1, 4, 2), (3, 5)), Cin=256),
    _c("qproj_stat", 1, 5, 70, 97, 64, ((10, 2, 2, 1, 3), (4, 0)), Cin=64),          # 4 key blocks beside the largest K tile
    _c("qproj_stat", 2, 5, 70, 77, 64, ((10, 2, 2, 1, 3), (3, 4)), Cin=64),
    _c("qproj_stat", 1, 5, 70, 32, 64, ((10, 2, 2, 1, 3), (1, 0)), Cin=64),
    _c("qproj_stat", 2, 5, 70, 64, 64, ((10, 1, 2, 2, 2), (2, 0)), Cin=128),
    _c("qproj_stat", 2, 5, 70, 5, 64, ((10, 1, 2, 2, 2), (1, 0)), Cin=128),
)
BY_NAME = {c.name: c for c in CASES}
KERNELS = ("qk_stats", "qk_parts", "long_qk_parts", "scope_head_parts", "qproj_stat")

# row scope: (B, H, N, M, D), M in {5, 33, 77, 97}
ROW_SHAPES = ((2, 2, 33, 5, 8), (2, 3, 70, 33, 40), (1, 2, 129, 77, 64), (2, 2, 70, 97, 160))
# fold of caller-made partials
FOLD_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 300)
FOLD_SHAPES = {"lean": (2, 2, 70, 64, 40), "general": (2, 2, 70, 33, 40)}         # (B, H, N, M, D): M >= 64 with bias_cols <= 64 / M < 64


SCOPE_FOLD_COUNTS = tuple(P for P in FOLD_COUNTS if P <= 256)      # (the scope library never forms more than 256 partials per (image, head))


def scope_fold_rows(P):
    """N with P <= 256 partials per (image, head) in pww_scope_cross_attn_fwd (which takes nothing but its own count)"""
    return 128 * P - 100


def case_form(case):
    """The form the dispatch model gives a case (for qproj_stat: tile + ring and statistic unit)"""
    if case.kernel == "qproj_stat":
        m = model_qproj(case.B, case.N, case.Cin, case.H, case.D, case.M)
        return None if m is None else (m[0], m[1])
    m = MODELS[case.kernel](case.B, case.H, case.N, case.M, case.D)
    return m if case.kernel == "qk_stats" else m[0]


def case_parts(case):
    """Partials per image (per (image, head) for scope_head_parts) by the model; None for qk_stats"""
    if case.kernel == "qk_stats":
        return None
    if case.kernel == "qproj_stat":
        return model_qproj(case.B, case.N, case.Cin, case.H, case.D, case.M)[2]
    return MODELS[case.kernel](case.B, case.H, case.N, case.M, case.D)[1]


def lane_chain(case):
    """L of the `shifted` bound: scores a lane adds in fp32 before it widens to fp64 -- 16 (one score block) in the partials kernels and in
    qproj_stat, 32 ceil(M / 64) in qk_reduce_kernel (vsum / vsq run over all key tiles of the lane's row). The real chains are a little
    longer (qproj_stat adds the blocks of a unit in fp32, qk_reduce_kernel the 64 lanes and the waves): the bound is the tighter for it."""
    return 32 * cdiv(case.M, 64) if case.kernel == "qk_stats" else 16


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------

def probe_positions(N, M):
    return ((N - 1, M - 1), (0, 0), (N - 1, 32 * ((M - 1) // 32)), (32 * ((N - 1) // 32), M - 1))


def probes(case):
    """Per image: ((row, key) of the near probe, (row, key) of the far probe or None). Image 0 of EVERY case has its near probe at
    (N - 1, M - 1); the images behind it take the other three positions in turn, starting at the case's index among its kernel's cases. The far probe takes the
    first of (N - 1, M - 1), (last row block, M - 1), (N - 1, last key block), (0, 0) that shares neither row nor key with the near one."""
    pos, off = probe_positions(case.N, case.M), [c for c in CASES if c.kernel == case.kernel].index(case)
    out = []
    for b in range(case.B):
        near = pos[0] if b == 0 else pos[1 + (b - 1 + off) % 3]
        far = next((f for f in (pos[0], pos[3], pos[2], pos[1]) if f[0] != near[0] and f[1] != near[1]), None)
        if case.shared:
            near, far = (near[0], case.M - 1), None
        out.append((near, far))
    return out


def _two(shape, lo, hi, g):
    return lo + (hi - lo) * torch.randint(0, 2, shape, generator=g).float()


def build(case, dtype, variant):
    """The inputs of one variant on the CPU: dict(q [B, N, H D], k [B or 1, M, H D] in `dtype`, heads; qproj_stat: also x [B, N, Cin] and
    w [H D, Cin] with q = x w^T exactly). `view` returns the probe_neg tensors: as_views() wraps them on the device they run on."""
    B, H, N, M, D = case.B, case.H, case.N, case.M, case.D
    C, Bk = H * D, 1 if case.shared else case.B
    g = torch.Generator().manual_seed(SEED + CASES.index(case))
    qp = case.kernel == "qproj_stat"
    rows = (B, N, case.Cin if qp else C)
    if variant == "shifted":
        x = 0.6 * torch.randn(rows, generator=g) + 0.4
        k = torch.randn(Bk, M, C, generator=g) + 0.5
    else:
        if variant == "view":
            variant = "probe_neg"
        sign = -1.0 if variant.endswith("neg") else 1.0
        x = _two(rows, 0.75, 1.0, g)
        k = sign * _two((Bk, M, C), 0.75, 1.0, g)
        if variant.startswith("probe"):
            for b, (near, far) in enumerate(probes(case)):
                x[b, near[0]], k[b if Bk > 1 else 0, near[1]] = NEAR, sign * NEAR
                if far is not None:
                    x[b, far[0]], k[b, far[1]] = FAR, sign * FAR
    out = dict(k=k.to(dtype), heads=H)
    if qp:
        w = torch.zeros(C, case.Cin)
        c = torch.arange(C)
        w[c, c % case.Cin] = 0.5
        w[c, (7 * c + 3) % case.Cin] = 0.5
        out["x"], out["w"] = x.to(dtype), w.to(dtype)
        out["q"] = (out["x"].double() @ out["w"].double().t()).to(dtype)
    else:
        out["q"] = x.to(dtype)
    return out


def to_device(inp, device):
    return {n: t.to(device) if torch.is_tensor(t) else t for n, t in inp.items()}


def as_views(inp):
    """q, k (and x) of `inp` as strided views [:, :rows, :cols] of NaN-filled [B, rows + PAD_ROWS, cols + PAD_COLS] buffers"""
    out = dict(inp)
    for n in ("q", "k", "x"):
        if n in inp:
            t = inp[n]
            buf = torch.full((t.shape[0], t.shape[1] + PAD_ROWS, t.shape[2] + PAD_COLS), float("nan"), dtype=t.dtype, device=t.device)
            buf[:, :t.shape[1], :t.shape[2]] = t
            out[n] = buf[:, :t.shape[1], :t.shape[2]]
    return out


# ---- fp64 reference ---------------------------------------------------------------------------------------------------------------------------

def _heads(t, B, H):
    t = t.double().expand(B, -1, -1)
    return t.reshape(B, t.shape[1], H, -1).permute(0, 2, 1, 3)


def scores(q, k, H):
    """fp64 Q K^T [B, H, N, M] of [B, N, H D] / [B or 1, M, H D] tensors, on their device"""
    B = q.shape[0]
    return _heads(q, B, H) @ _heads(k, B, H).transpose(-1, -2)


def abs_scores(q, k, H):
    """sum_d |q_nd| |k_md|, the scale of the forward rounding bound of a score"""
    return scores(q.abs(), k.abs(), H)


def fields(s, scope="image"):
    """(max, min, sum, sum of squares) of the fp64 scores s [B, H, N, M]: image -> [B, 4], head -> [B, H, 4]; an empty s gives the neutral
    element (-inf, +inf, 0, 0)"""
    dims = (1, 2, 3) if scope == "image" else (2, 3)
    if s.numel() == 0:
        shape = (s.shape[0],) if scope == "image" else s.shape[:2]
        return torch.tensor([-math.inf, math.inf, 0.0, 0.0], dtype=torch.float64, device=s.device).expand(*shape, 4).clone()
    return torch.stack([s.amax(dims), s.amin(dims), s.sum(dims), (s * s).sum(dims)], dim=-1)


FAULTS = ("padding_leak", "last_key_excluded", "last_row_excluded", "tail_rows_duplicated")


def emulate(s, fault):
    """The scores a faulty kernel would reduce: padding_leak -- zeros up to whole 32-row and 32-key blocks take part in the extremes;
    last_key_excluded / last_row_excluded; tail_rows_duplicated -- rows N .. 32 ceil(N / 32) - 1 repeat row N - 1"""
    N, M = s.shape[-2:]
    if fault == "padding_leak":
        return torch.nn.functional.pad(s, (0, cdiv(M, 32) * 32 - M, 0, cdiv(N, 32) * 32 - N))
    if fault == "last_key_excluded":
        return s[..., :M - 1]
    if fault == "last_row_excluded":
        return s[..., :N - 1, :]
    return torch.cat([s, s[..., N - 1:, :].expand(*s.shape[:2], cdiv(N, 32) * 32 - N, M)], dim=-2)


def sum_bars(s, variant, case, q=None, k=None):
    """(bar of the sum, bar of the sum of squares), each shaped like fields(s)[..., 0]. Dyadic variants: the bars of the existing tests,
    1e-6 cnt max|s| and 1e-6 of the reference. shifted: the forward rounding bound with u = 2^-24 and L = lane_chain(case):
    (D + L + 2) u sum(|q| . |k|) and (2 D + L + 4) u sum(s^2)."""
    scope = "head" if case.kernel == "scope_head_parts" else "image"
    dims = (1, 2, 3) if scope == "image" else (2, 3)
    f = fields(s, scope)
    if variant != "shifted":
        cnt = s.numel() // f[..., 0].numel()
        return 1e-6 * cnt * s.abs().amax(dims), 1e-6 * f[..., 3]
    L = lane_chain(case)
    return (case.D + L + 2) * U * abs_scores(q, k, case.H).sum(dims), (2 * case.D + L + 4) * U * f[..., 3]


def mean_std(f, cnt):
    """mean and unbiased standard deviation from (sum, sum of squares) fields, as the attention kernels form them"""
    mean = f[..., 2] / cnt
    var = (f[..., 3] - f[..., 2] * mean) / (cnt - 1) if cnt > 1 else torch.zeros_like(mean)
    return mean, var.clamp_min(0).sqrt()


# ---- row scope --------------------------------------------------------------------------------------------------------------------------------

def row_inputs(shape, dtype, variant):
    """q, k, v, the map and the scalar of a row-scope call: dyadic one-signed q / k, Gaussian v, a map with weights near 1 in the columns
    0, 3 and M - 1 of 60 % of the rows, scalar 8 / sqrt(D): scalar * 0.25 D * scale = 2"""
    B, H, N, M, D = shape
    g = torch.Generator().manual_seed(SEED + 500 + sum(shape))
    sign = -1.0 if variant == "neg" else 1.0
    q = _two((B, N, H * D), 0.75, 1.0, g).to(dtype)
    k = (sign * _two((1, M, H * D), 0.75, 1.0, g)).to(dtype)
    v = torch.randn(1, M, H * D, generator=g).to(dtype)
    w = torch.zeros(N, M)
    for c in sorted({0, min(3, M - 1), M - 1}):
        rows = torch.rand(N, generator=g) < 0.6
        w[rows, c] = 0.9 + 0.2 * float(torch.rand((), generator=g))
    return dict(q=q, k=k, v=v, w=w, heads=H, scale=D ** -0.5, scalar=8.0 / math.sqrt(D))


def row_stat(s, kind, leak=False):
    """The statistic of every row of the fp64 scores s [B, H, N, M] -> [B, H, N, 1]; kind: "MAX", "MIN", "MEAN", "STD", "ABSMAX".
    leak: the extremes also see the zeros that pad the row to whole 32-key blocks."""
    e = emulate(s, "padding_leak")[..., :s.shape[-2], :] if leak else s
    if kind == "MAX":
        return e.amax(-1, keepdim=True)
    if kind == "MIN":
        return e.amin(-1, keepdim=True)
    if kind == "ABSMAX":
        return e.abs().amax(-1, keepdim=True)
    return s.mean(-1, keepdim=True) if kind == "MEAN" else s.std(-1, keepdim=True)


def row_oracle(inp, kind, leak=False):
    """softmax((Q K^T + scalar * stat(row) * w) scale) V in fp64 on the rounded inputs -> [B, N, H D]"""
    H, B = inp["heads"], inp["q"].shape[0]
    s = scores(inp["q"], inp["k"], H)
    p = ((s + inp["scalar"] * row_stat(s, kind, leak) * inp["w"].double()) * inp["scale"]).softmax(-1)
    return (p @ _heads(inp["v"], B, H)).permute(0, 2, 1, 3).reshape(B, s.shape[2], -1)


# ---- synthetic partials -------------------------------------------------------------------------------------------------------------------------

def synthetic_parts(lead, P, seed):
    """fp64 partials [*lead, P, 4] with float-representable values: maxima negative, minima positive, both extremes in the LAST partial,
    every third partial (never the last) the neutral element (-inf, +inf, 0, 0); sums negative, sums of squares positive and far above sum^2 / count (a standard deviation exists)"""
    g = torch.Generator().manual_seed(SEED + 900 + seed)
    r = torch.rand(*lead, P, 4, generator=g).double()          # (fp32 draws: exact as floats)
    parts = torch.stack([-(1.0 + 9.0 * r[..., 0]), 1.0 + 9.0 * r[..., 1], -10.0 * r[..., 2], 1000.0 * r[..., 3]], dim=-1)
    parts = parts.float().double()
    parts[..., P - 1, 0], parts[..., P - 1, 1] = -0.5, 0.25
    neutral = torch.tensor([-math.inf, math.inf, 0.0, 0.0], dtype=torch.float64)
    idx = [i for i in range(P - 1) if i % 3 == 1]
    parts[..., idx, :] = neutral
    return parts


def fold(parts):
    """[..., P, 4] -> [..., 4] in torch"""
    return torch.stack([parts[..., 0].amax(-1), parts[..., 1].amin(-1), parts[..., 2].sum(-1), parts[..., 3].sum(-1)], dim=-1)
