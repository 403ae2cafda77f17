"""Case table and probe inputs of the general attention launch (csrc/pww_attn_kernel.h: dispatch_nw, dispatch_d, launch_attn), one case per
code object the dispatch can reach, and the fp64 reference they are compared with. Plain torch, no GPU code: test_attn_routes_host.py checks
the table and the inputs on the CPU, test_attn_routes_gpu.py runs ops.attention on them.

A route is the record of pww_debug_last_attn_route: (kind, KS, DT, NW, KG, NSUB, HAS_BIAS, ROWSUM_MFMA, RF).
  kind         GENERAL (attn_fwd_kernel), KSPLIT (the same kernel with KG key groups), FOLD (attn_fwd_fold_kernel, d = 8 / 24 / 40)
  (KS, DT)     head-dim class: D <= 48 (3, 2), <= 64 (4, 2), <= 80 (5, 3), <= 96 (6, 3), <= 128 (8, 4), <= 160 (10, 5)
  NW           row groups of 32 query rows: 2, 4 or 8, from rows32 = ceil(N / 32) B H (SHAPES below sit on the thresholds)
  NSUB         64-key sub-tiles per stage: general kernel 2 for (3, 2) and 1 above it; key-split kernel KG; folded kernel 2
  ROWSUM_MFMA  the softmax denominator comes from a ones column of V (no bias and D % 32 != 0; always in the folded kernel)
  RF           range-free softmax (no bias, NW >= 4; the folded kernel in both storage types)
The same shape takes the same route in fp16 and bf16.

Inputs. q and k are independent Gaussian tensors (N != M; scale = D^-0.5, so the scaled logits have unit spread), v is Gaussian with
standard deviation V_STD. On top of them sit spike probes: in every (image, head) each probe row -- 0, 31, 32, 64, N - 2, N - 1: first and last
row of a wave, first row of the second and third wave, the two last valid rows of the ragged last block -- points at ONE probe key -- M - 1,
M - 2, 0 or the first key of the last 64-key tile, dealt round-robin and rotated from head to head. The query row is set parallel to the
(rounded) key with a scaled logit of exactly `logit`, the key's v row is 4.0. A probe key is rescaled to a norm of max(sqrt(D), PROBE_NORM):
the probe row's logits against the other keys then have a spread of logit / |k| <= 6 / 7, so that the probe key holds a known share of its
row whatever the head dim (a plain Gaussian key of D = 8 would leave a spread of 2.1 and a share of 7 % at M = 577). The probe keys of
a head are orthogonal to each other (Gaussian directions through a QR step): a probe row sees the other probe keys -- key M - 1 with the
bias spike among them -- at logit 0.

V_STD = 0.125 is chosen so that the condition test_attn_routes_host.py checks can hold in bf16 at all: dropping a key that holds the share
p moves the row by p (4 - a) with a the other keys' mean, against a per-row bar of TOL s_n with s_n = 4 p + (1 - p) E|v|. At p = 0.167
(M = 1217) and unit-variance v the ratio is 0.5 / TOL = 31 bars in bf16; with E|v| = 0.1 it is 0.89 / TOL = 55 bars.

Variants (build()):
  mild     probes with logit 6
  strong   probes with logit 16 (2^23 in the exp2 domain: past the fp16 range of an un-referenced P)
  classes  the mild q and k; v in {0, 1}: column c < NCLS of key m is one iff class(m) == c, the keys of the last 64-key tile are class
           NCLS - 1, the others (m * 5 + head) % (NCLS - 1). O[:, c] is then the probability mass of class c and columns 0 .. NCLS - 1 sum to 1.
  view     the mild tensors as strided views (as_views()): rows behind the last key / query row hold NaN, the columns beside k and v hold
           +-6e4 (fp16) / +-1e30 (bf16)
Biased cases add a sparse fp32 [N, M] map (5 % of the entries, scaled contribution below 1) with the entries [0, M - 1] and [N - 1, M - 1] --
the last word the bias descriptor covers -- at a scaled contribution of 6, and per-image coefficients BIAS_COEFF (1, 0.5, 0, 1).
"""
import collections
import functools
import math

import torch

GENERAL, KSPLIT, FOLD = 1, 2, 3
ROUTE_FIELDS = ("kind", "KS", "DT", "NW", "KG", "NSUB", "HAS_BIAS", "ROWSUM_MFMA", "RF")

# (B, H, N) per workgroup width. NW = 2: the last workgroup holds 2 rows and its second wave none. NW = 4: rows32 = 1024 exactly (the threshold)
# and ceil(N / 128) B H = 256 exactly (the key-split 4 x 3 threshold); the last wave of the last block holds 8 rows. NW = 8: rows32 = 2048 exactly.
SHAPES = {2: (1, 2, 130), 4: (4, 8, 1000), 8: (8, 8, 1000)}

Case = collections.namedtuple("Case", "name nw D M bias route")


def _c(nw, D, M, route, bias=False):
    kind = {GENERAL: "bias" if bias else "gen", KSPLIT: "ks%dx%d" % (route[3], route[4]), FOLD: "fold"}[route[0]]
    return Case("nw%d_%s_d%d_m%d" % (nw, kind, D, M), nw, D, M, bias, route)


CASES = (
    # ---- 2-wave workgroups (no range-free mode) ----
    _c(2, 8, 200, (FOLD, 3, 2, 2, 1, 2, 0, 1, 1)),
    _c(2, 16, 577, (GENERAL, 3, 2, 2, 1, 2, 0, 1, 0)),
    _c(2, 32, 200, (GENERAL, 3, 2, 2, 1, 2, 0, 0, 0)),
    _c(2, 56, 577, (GENERAL, 4, 2, 2, 1, 1, 0, 1, 0)),
    _c(2, 64, 200, (GENERAL, 4, 2, 2, 1, 1, 0, 0, 0)),
    _c(2, 72, 200, (GENERAL, 5, 3, 2, 1, 1, 0, 1, 0)),        # (M < 512: below the key-split 2 x 2 threshold)
    _c(2, 80, 600, (KSPLIT, 5, 3, 2, 2, 2, 0, 1, 0)),
    _c(2, 88, 200, (GENERAL, 6, 3, 2, 1, 1, 0, 1, 0)),
    _c(2, 96, 200, (GENERAL, 6, 3, 2, 1, 1, 0, 0, 0)),
    _c(2, 88, 577, (KSPLIT, 6, 3, 2, 2, 2, 0, 1, 0)),
    _c(2, 96, 576, (KSPLIT, 6, 3, 2, 2, 2, 0, 0, 0)),         # (the second key group sees nothing in the tail)
    # ---- 4-wave workgroups ----
    _c(4, 24, 577, (FOLD, 3, 2, 4, 1, 2, 0, 1, 1)),
    _c(4, 48, 1217, (KSPLIT, 3, 2, 4, 3, 3, 0, 1, 0)),        # (tail of 65: group 0 a full tile, group 1 one key, group 2 nothing)
    _c(4, 32, 1024, (KSPLIT, 3, 2, 4, 3, 3, 0, 0, 0)),        # (tail of exactly 64 on the ragged path)
    _c(4, 16, 577, (GENERAL, 3, 2, 4, 1, 2, 0, 1, 1)),
    _c(4, 32, 200, (GENERAL, 3, 2, 4, 1, 2, 0, 0, 1)),
    _c(4, 56, 1024, (KSPLIT, 4, 2, 4, 3, 3, 0, 1, 0)),
    _c(4, 64, 1217, (KSPLIT, 4, 2, 4, 3, 3, 0, 0, 0)),
    _c(4, 56, 200, (GENERAL, 4, 2, 4, 1, 1, 0, 1, 1)),
    _c(4, 64, 577, (GENERAL, 4, 2, 4, 1, 1, 0, 0, 1)),
    _c(4, 80, 577, (GENERAL, 5, 3, 4, 1, 1, 0, 1, 1)),
    _c(4, 88, 200, (GENERAL, 6, 3, 4, 1, 1, 0, 1, 1)),
    _c(4, 96, 577, (GENERAL, 6, 3, 4, 1, 1, 0, 0, 1)),
    _c(4, 120, 577, (GENERAL, 8, 4, 4, 1, 1, 0, 1, 1)),       # (D % 32 = 24: the row-sum register of the last d-tile's upper half)
    _c(4, 128, 200, (GENERAL, 8, 4, 4, 1, 1, 0, 0, 1)),
    _c(4, 152, 200, (GENERAL, 10, 5, 4, 1, 1, 0, 1, 1)),      # (D % 32 = 24)
    _c(4, 160, 577, (GENERAL, 10, 5, 4, 1, 1, 0, 0, 1)),
    # ---- 8-wave workgroups (D <= 64) ----
    _c(8, 40, 200, (FOLD, 3, 2, 8, 1, 2, 0, 1, 1)),
    _c(8, 48, 200, (GENERAL, 3, 2, 8, 1, 2, 0, 1, 1)),
    _c(8, 32, 577, (GENERAL, 3, 2, 8, 1, 2, 0, 0, 1)),
    _c(8, 56, 577, (GENERAL, 4, 2, 8, 1, 1, 0, 1, 1)),
    _c(8, 64, 200, (GENERAL, 4, 2, 8, 1, 1, 0, 0, 1)),
    # ---- biased (2 or 4 waves; row sum on the VALU, running-maximum softmax) ----
    _c(2, 40, 77, (GENERAL, 3, 2, 2, 1, 2, 1, 0, 0), bias=True),
    _c(2, 64, 77, (GENERAL, 4, 2, 2, 1, 1, 1, 0, 0), bias=True),
    _c(2, 72, 77, (GENERAL, 5, 3, 2, 1, 1, 1, 0, 0), bias=True),
    _c(2, 88, 77, (GENERAL, 6, 3, 2, 1, 1, 1, 0, 0), bias=True),
    _c(4, 48, 130, (GENERAL, 3, 2, 4, 1, 2, 1, 0, 0), bias=True),
    _c(4, 56, 77, (GENERAL, 4, 2, 4, 1, 1, 1, 0, 0), bias=True),
    _c(4, 80, 130, (GENERAL, 5, 3, 4, 1, 1, 1, 0, 0), bias=True),
    _c(4, 96, 77, (GENERAL, 6, 3, 4, 1, 1, 1, 0, 0), bias=True),
    _c(4, 104, 130, (GENERAL, 8, 4, 4, 1, 1, 1, 0, 0), bias=True),
    _c(4, 160, 77, (GENERAL, 10, 5, 4, 1, 1, 1, 0, 0), bias=True),
)
BY_NAME = {c.name: c for c in CASES}

DTYPES = (torch.float16, torch.bfloat16)
VARIANTS = ("mild", "strong", "classes", "view")
LOGIT = {"mild": 6.0, "strong": 16.0, "classes": 6.0, "view": 6.0}
SEED = 20240
V_STD, V_PROBE, PROBE_NORM = 0.125, 4.0, 7.0
NCLS = 8
BIAS_COEFF = (1.0, 0.5, 0.0, 1.0)
BIAS_SPIKE = 6.0
PAD_ROWS = 64
HUGE = {torch.float16: 6e4, torch.bfloat16: 1e30}


def probe_rows(N):
    return (N - 1, 0, 31, 32, 64, N - 2)


def probe_keys(M):
    """M - 1, M - 2, key 0, first key of the last 64-key tile (partial, or the full one a multiple of 64 ends with)."""
    return (M - 1, M - 2, 0, (M - 1) // 64 * 64)


def probes(case):
    """(head index over B * H, row, key) of every probe: row i of head j points at key (i + j) % 4. Biased cases: rows 0 and N - 1, which
    carry the bias spike at key M - 1, always point at that key (two keys with the same v row in one probe row would stand in for each other)."""
    B, H, N = SHAPES[case.nw]
    rows, keys = probe_rows(N), probe_keys(case.M)
    return [(j, r, keys[0 if case.bias and r in (0, N - 1) else (i + j) % len(keys)]) for j in range(B * H) for i, r in enumerate(rows)]


def key_class(M, H):
    """[H, M] int64: the class of every key in the `classes` variant."""
    m = torch.arange(M)
    cls = (m[None, :] * 5 + torch.arange(H)[:, None]) % (NCLS - 1)
    cls[:, (M - 1) // 64 * 64:] = NCLS - 1
    return cls


@functools.lru_cache(maxsize=1)
def _base(name):
    """fp32 Gaussian q [B, N, H, D], k and v [B, M, H, D] of a case with the probe keys at their norm, and the bias map: what every storage
    type and variant starts from."""
    case = BY_NAME[name]
    B, H, N = SHAPES[case.nw]
    D, M = case.D, case.M
    g = torch.Generator().manual_seed(SEED + CASES.index(case))
    q = torch.randn(B, N, H, D, generator=g)
    k = torch.randn(B, M, H, D, generator=g)
    v = torch.randn(B, M, H, D, generator=g) * V_STD
    keys = sorted(set(probe_keys(M)))
    ortho = torch.linalg.qr(k[:, keys].permute(0, 2, 3, 1)).Q                     # [B, H, D, keys]: orthonormal columns
    k[:, keys] = ortho.permute(0, 3, 1, 2) * max(math.sqrt(D), PROBE_NORM)
    bias = None
    if case.bias:
        scale = D ** -0.5
        bias = (torch.rand(N, M, generator=g) < 0.05).float() * torch.rand(N, M, generator=g) / scale
        bias[0, M - 1] = bias[N - 1, M - 1] = BIAS_SPIKE / scale
    return q, k, v, bias


def build(case, dtype, variant):
    """The inputs of one variant on the CPU: dict(q [B, N, H D], k, v [B, M, H D] in `dtype`, bias fp32 [N, M] or None, coeff fp32 [B] or
    None, heads, scale). `view` returns the mild tensors: as_views() wraps them on the device they run on."""
    B, H, N = SHAPES[case.nw]
    D, M = case.D, case.M
    q, k, v, bias = _base(case.name)
    scale = D ** -0.5
    kT = k.to(dtype).float()
    q = q.clone()
    j, r, m = (torch.tensor(t) for t in zip(*probes(case)))
    b, h = j // H, j % H
    kp = kT[b, m, h]                                        # [P, D]
    q[b, r, h] = kp * (LOGIT[variant] / (scale * (kp * kp).sum(-1, keepdim=True)))
    if variant == "classes":
        v = (key_class(M, H)[:, :, None] == torch.arange(D)[None, None, :]).float().transpose(0, 1)[None].expand(B, M, H, D)
    else:
        v = v.clone()
        v[:, sorted(set(probe_keys(M)))] = V_PROBE
    coeff = torch.tensor([BIAS_COEFF[i % len(BIAS_COEFF)] for i in range(B)]) if case.bias else None
    return dict(q=q.to(dtype).reshape(B, N, H * D), k=kT.to(dtype).reshape(B, M, H * D), v=v.to(dtype).reshape(B, M, H * D).contiguous(),
                bias=bias, coeff=coeff, heads=H, scale=scale)


def to_device(inp, device):
    return {n: t.to(device) if torch.is_tensor(t) else t for n, t in inp.items()}


def as_views(inp):
    """q, k and v of `inp` as strided views of larger buffers: PAD_ROWS rows of NaN behind the last query row / key, and k and v as the
    middle third of the columns of a buffer whose other columns hold +-HUGE."""
    out = dict(inp)
    q = inp["q"]
    B, N, C = q.shape
    qbuf = torch.full((B, N + PAD_ROWS, C), float("nan"), dtype=q.dtype, device=q.device)
    qbuf[:, :N] = q
    out["q"] = qbuf[:, :N]
    for n in ("k", "v"):
        t = inp[n]
        M = t.shape[1]
        buf = torch.full((B, M + PAD_ROWS, 3 * C), float("nan"), dtype=t.dtype, device=t.device)
        sign = 1.0 - 2.0 * ((torch.arange(M, device=t.device)[:, None] + torch.arange(3 * C, device=t.device)[None, :]) % 2)
        buf[:, :M] = (sign * HUGE[t.dtype]).to(t.dtype)
        buf[:, :M, C:2 * C] = t
        out[n] = buf[:, :M, C:2 * C]
    return out


def reference(inp, b, rows=None):
    """Image b in fp64 on the tensors' device: O [H, n, D], s [H, n] with s_n = max_c sum_m p_nm |v_mc| (the scale of the per-row bar) and the
    probabilities p [H, n, M]; rows: the query rows to compute (default: all)."""
    H, scale = inp["heads"], inp["scale"]
    q, k, v = (inp[n][b].double() for n in ("q", "k", "v"))
    if rows is not None:
        q = q[rows]
    qh, kh, vh = (t.reshape(t.shape[0], H, -1).transpose(0, 1) for t in (q, k, v))
    logits = torch.matmul(qh, kh.transpose(-1, -2))
    if inp["bias"] is not None:
        bias = inp["bias"].double()
        logits = logits + inp["coeff"][b].double() * (bias if rows is None else bias[rows])[None]
    p = (logits * scale).softmax(-1)
    return torch.matmul(p, vh), torch.matmul(p, vh.abs()).max(-1).values, p
