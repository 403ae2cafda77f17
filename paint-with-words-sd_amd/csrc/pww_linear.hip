// Linear layers on gfx950 MFMA with the post-processing of the GEMM's output in its epilogue (pww_linear_fwd):
//
//   y[m, n] = epilogue(sum_k x[m, k] * w[n, k]),   x [M, K] with a row stride,  w [N, K] an nn.Linear / 1 x 1 conv weight, used in place
//
// The tile and the K loop are those of pww_conv.hip (3 x 3 convolution) with the gather removed: 128 (M) x BN (64 or 128) x 64 (K) per
// 256-thread workgroup, 2 x 2 waves, mfma_f32_16x16x32 with the WEIGHT as the A operand (a lane holds 4 consecutive output channels of one
// row), LDS rows of 128 bytes with the 16-byte chunk index XOR-ed by (row & 7), LN_PF K-slabs of global loads in flight in register sets,
// counted vmcnt waits, a steady loop without conditions unrolled LN_PF times, the XCD-aware tile order. The loop is WRITTEN AGAIN here:
// moving it into a header that both units include changed the register allocation and the wait counts of the convolution's code objects
// (218 instead of 220 VGPRs, other vmcnt values), and those are what its measured times rest on.
// The M tail loads from clamped rows and masks the store: no load sits under a condition.
//
// Epilogues (one code object per (T, BN), a uniform branch at the store). BIAS rounds the accumulator, then the sum (one rounding more than a
// GEMM whose own epilogue adds the bias); on that result RESIDUAL and GEGLU have the rounding points of the unfused sequence on T tensors:
//   NONE            T(acc)
//   BIAS            T(T(acc) + b[n])
//   BIAS_RESIDUAL   T(r[m, n] + T(T(acc) + b[n]))                              `lin(x) + r`; r has its own row stride, y may alias r
//   BIAS_GEGLU      N = 2 inner, y [M, inner]:  y[m, j] = T(hv * T(gelu(hg))),  hv = T(T(acc[m, j]) + b[j]),  hg = T(T(acc[m, inner + j]) + b[inner + j])
//                   (erf form: pww_geglu's formula). A workgroup's BN tile rows are BN / 2 value rows of w and the BN / 2 gate rows `inner`
//                   further on, laid out so that each lane ends up with a value and its gate: no repacked weight.
//
// Split-K: each workgroup writes its fp32 partial tile to a caller-owned workspace ([split][M][N]), a second launch folds the partials in
// split order and applies the same epilogue (GEGLU included). No atomics, no inter-workgroup waits: bitwise repeatable.
//
// Built as a library of its own (libpww_hip_linear.so, include/pww_hip_linear.h): the unit is self-contained, its host plumbing is pww_side_host.h, and
// only the pww_linear_* entry points are visible (compiled with -fvisibility=hidden).
#define PWW_SIDE_LIB "libpww_hip_linear"
#include "pww_side_host.h"
#include "../../include/pww_hip_linear.h"

#define PWW_LINEAR_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int LN_BM = 128, LN_THREADS = 256;
constexpr int LN_PF = 2;        // K-slabs of global loads in flight while one is computed (pww_conv.hip: CV_PF)

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// cold kernel arguments (behind the preloaded hot ones)
struct LinCold {
    const void *bias, *residual;
    long ys, rs;            // row strides of y and the residual, in elements
    int nsplit, nslab, mode, inner;
    int through;            // split launches: the partials are stored write-through (pww_common.h: store_partial_through)
};

// bijective block-id remap: consecutive logical ids (tiles that share weight columns) on one XCD (guide T1)
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

template <typename T> __device__ __forceinline__ float rnd(float v) { return (float)(T)v; }

// NONE / BIAS / BIAS_RESIDUAL of 4 consecutive channels n .. n + 3 of row m
template <typename T>
__device__ __forceinline__ void epilogue4(const f32x4 &a, const LinCold &cold, T *y, int m, int n) {
    typedef typename Vec<T>::v4 V4;
    V4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)a[j];
    if (cold.mode >= PWW_LINEAR_BIAS) {
        const V4 b = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias) + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (T)((float)o[j] + (float)b[j]);
    }
    if (cold.mode == PWW_LINEAR_BIAS_RESIDUAL) {
        const V4 r = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.residual) + (long)m * cold.rs + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (T)((float)r[j] + (float)o[j]);
    }
    *reinterpret_cast<V4 *>(y + (long)m * cold.ys + n) = o;
}

// BIAS_GEGLU of the 4 output channels j0 .. j0 + 3 of row m: av = the value accumulators, ag = their gates
template <typename T>
__device__ __forceinline__ void geglu4(const f32x4 &av, const f32x4 &ag, const LinCold &cold, T *y, int m, int j0) {
    typedef typename Vec<T>::v4 V4;
    const V4 bv = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias) + j0);
    const V4 bg = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias) + cold.inner + j0);
    V4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float hv = rnd<T>(rnd<T>(av[j]) + (float)bv[j]);
        const float g = rnd<T>(rnd<T>(ag[j]) + (float)bg[j]);
        const float ge = rnd<T>(0.5f * g * (1.f + erff(g * 0.70710678118654752440f)));      // F.gelu (erf form) on a T tensor
        o[j] = (T)(hv * ge);
    }
    *reinterpret_cast<V4 *>(y + (long)m * cold.ys + j0) = o;
}

// Hot arguments first: 10 dwords preloaded into SGPRs. xs = row stride of x in elements.
template <typename T, int BN>
__global__ void __launch_bounds__(LN_THREADS, 2) linear_kernel(const T *__restrict__ x, const T *__restrict__ w, void *out, int M, int N, int K, int xs,
                                                               const LinCold cold) {
    typedef typename Vec<T>::v8 V8;
    constexpr int BM = LN_BM, PF = LN_PF, XL = BM * 8 / LN_THREADS, WL = BN * 8 / LN_THREADS, RM = 4, RN = BN / 32;
    constexpr int XBYTES = BM * 128, STAGE = (BM + BN) * 128;
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int ntm = (M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const bool split = cold.nsplit > 1;                     // (uniform: one code object serves both)
    const bool geglu = cold.mode == PWW_LINEAR_BIAS_GEGLU;  // (uniform)
    const int tile = bid / cold.nsplit, ks = bid - tile * cold.nsplit;
    const int tm = tile % ntm, tn = tile / ntm;
    const int s_begin = (int)((long)ks * cold.nslab / cold.nsplit), s_end = (int)((long)(ks + 1) * cold.nslab / cold.nsplit);

    // this thread's XL rows of x and WL rows of w (tile row (tid >> 3) + 32 i, 16-byte chunk tid & 7 of the slab). GEGLU: the tile's half wn
    // holds BN / 4 value rows, then their BN / 4 gate rows (`inner` further on in w), so that MFMA sub-tile r and r + RN / 2 of a wave pair up.
    const int c = tid & 7;
    unsigned xoff[XL], woff[WL];
#pragma unroll
    for (int i = 0; i < XL; ++i) {
        int m = tm * BM + (tid >> 3) + 32 * i;
        m = m < M ? m : M - 1;
        xoff[i] = (unsigned)(m * xs + c * 8);
    }
#pragma unroll
    for (int j = 0; j < WL; ++j) {
        const int t = (tid >> 3) + 32 * j;
        const int u = t % (BN / 2);
        const int row = geglu ? (u >= BN / 4 ? cold.inner : 0) + tn * (BN / 2) + (t / (BN / 2)) * (BN / 4) + u % (BN / 4) : tn * BN + t;
        woff[j] = (unsigned)(row * K + c * 8);
    }
    const int swz = ((c ^ ((tid >> 3) & 7)) << 4);          // LDS byte offset of this thread's chunk within its row

    // PF register sets, one K-slab of global loads each: set p holds slab i + p (mod PF) while slab i is computed
    u32x4 xr[PF][XL], wr[PF][WL];
    const T *xnext = x + s_begin * 64, *wnext = w + s_begin * 64;
    auto load = [&](int p) {                               // the next slab in K order into set p
#pragma unroll
        for (int i = 0; i < XL; ++i) xr[p][i] = *reinterpret_cast<const u32x4 *>(xnext + xoff[i]);
#pragma unroll
        for (int j = 0; j < WL; ++j) wr[p][j] = *reinterpret_cast<const u32x4 *>(wnext + woff[j]);
        xnext += 64;
        wnext += 64;
    };
    auto store = [&](int p, int buf) {
        char *base = lds + buf * STAGE;
#pragma unroll
        for (int i = 0; i < XL; ++i) *reinterpret_cast<u32x4 *>(base + ((tid >> 3) + 32 * i) * 128 + swz) = xr[p][i];
#pragma unroll
        for (int j = 0; j < WL; ++j) *reinterpret_cast<u32x4 *>(base + XBYTES + ((tid >> 3) + 32 * j) * 128 + swz) = wr[p][j];
    };

    f32x4 acc[RN][RM];
#pragma unroll
    for (int r = 0; r < RN; ++r)
#pragma unroll
        for (int i = 0; i < RM; ++i) acc[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    auto compute = [&](int buf) {
        const char *bx = lds + buf * STAGE, *bw = bx + XBYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            V8 xf[RM], wf[RN];
#pragma unroll
            for (int q = 0; q < RM; ++q) {
                const int row = wm * 64 + q * 16 + fr;
                xf[q] = *reinterpret_cast<const V8 *>(bx + row * 128 + (((kk * 4 + fq) ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const int row = wn * (BN / 2) + r * 16 + fr;
                wf[r] = *reinterpret_cast<const V8 *>(bw + row * 128 + (((kk * 4 + fq) ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int r = 0; r < RN; ++r)
#pragma unroll
                for (int q = 0; q < RM; ++q) acc[r][q] = mfma16(wf[r], xf[q], acc[r][q]);
        }
    };

    // Slab i of this workgroup's n (>= 1: the host never plans more splits than slabs) lives in register set i % PF until it moves to LDS
    // buffer i & 1. Prologue: slabs 0 .. PF - 1 are requested, slab 0 lands in LDS (its wait counts past the younger sets' loads).
    const int n = s_end - s_begin;
    load(0);
#pragma unroll
    for (int p = 1; p < PF; ++p)
        if (p < n) load(p);
    store(0, 0);
    __syncthreads();
    // Slab i: request slab i + PF into the set slab i came from, compute slab i from LDS, move slab i + 1 (requested PF - 1 slabs ago) from
    // its registers to the other LDS buffer, one barrier. The steady loop is free of conditions, so the compiler's wait counts are exact.
    int i = 0;
    for (; i + 2 * PF <= n; i += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            load(p);
            compute((i + p) & 1);
            store((p + 1) % PF, (i + p + 1) & 1);
            __syncthreads();
        }
    }
    // drain: the last PF .. 2 PF - 1 slabs (or all of a short split), each request and move under its own condition
#pragma unroll
    for (int t = 0; t < 2 * PF - 1; ++t) {
        if (i + t < n) {
            if (i + t + PF < n) load(t % PF);
            compute((i + t) & 1);
            if (i + t + 1 < n) store((t + 1) % PF, (i + t + 1) & 1);
            __syncthreads();
        }
    }

    // lane holds D[tile row = wn BN / 2 + 16 r + 4 fq + j][m = 16 i + fr] of its wave's sub-tile
    if (split && cold.through) {                            // (uniform) the partials written through: pww_common.h, store_partial_through
        const unsigned ws_bytes = (unsigned)cold.nsplit * (unsigned)M * (unsigned)N * 4u;      // (the host asks for this only below 4 GiB)
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            const int m = tm * BM + wm * 64 + i * 16 + fr;
            if (m >= M) continue;
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const int col = geglu ? (r >= RN / 2 ? cold.inner : 0) + tn * (BN / 2) + wn * (BN / 4) + (r % (RN / 2)) * 16 + fq * 4
                                      : tn * BN + wn * (BN / 2) + r * 16 + fq * 4;
                store_partial_through(out, ws_bytes, (((unsigned)ks * (unsigned)M + (unsigned)m) * (unsigned)N + (unsigned)col) * 4u, acc[r][i]);
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < RM; ++i) {
        const int m = tm * BM + wm * 64 + i * 16 + fr;
        if (m >= M) continue;
        if (split) {
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const int col = geglu ? (r >= RN / 2 ? cold.inner : 0) + tn * (BN / 2) + wn * (BN / 4) + (r % (RN / 2)) * 16 + fq * 4
                                      : tn * BN + wn * (BN / 2) + r * 16 + fq * 4;
                *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(out) + ((long)ks * M + m) * N + col) = acc[r][i];
            }
        } else if (geglu) {
#pragma unroll
            for (int r = 0; r < RN / 2; ++r)
                geglu4<T>(acc[r][i], acc[r + RN / 2][i], cold, reinterpret_cast<T *>(out), m, tn * (BN / 2) + wn * (BN / 4) + r * 16 + fq * 4);
        } else {
#pragma unroll
            for (int r = 0; r < RN; ++r) epilogue4<T>(acc[r][i], cold, reinterpret_cast<T *>(out), m, tn * BN + wn * (BN / 2) + r * 16 + fq * 4);
        }
    }
}

// fold the split-K partials [nsplit][M][N] in split order, then the epilogue: one thread per 4 output channels of one row
template <typename T>
__global__ void __launch_bounds__(256) linear_fold_kernel(const float *__restrict__ ws, T *y, long n4, int N, long MN, const LinCold cold) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    const bool geglu = cold.mode == PWW_LINEAR_BIAS_GEGLU;
    const int nout = geglu ? cold.inner : N;
    const long o4 = q * 4;
    const int m = (int)(o4 / nout), n = (int)(o4 - (long)m * nout);
    const float *p = ws + (long)m * N + n;
    f32x4 a = *reinterpret_cast<const f32x4 *>(p);
    for (int s = 1; s < cold.nsplit; ++s) a += *reinterpret_cast<const f32x4 *>(p + s * MN);
    if (geglu) {
        f32x4 g = *reinterpret_cast<const f32x4 *>(p + cold.inner);
        for (int s = 1; s < cold.nsplit; ++s) g += *reinterpret_cast<const f32x4 *>(p + s * MN + cold.inner);
        geglu4<T>(a, g, cold, y, m, n);
    } else {
        epilogue4<T>(a, cold, y, m, n);
    }
}

// Tile width and K split per GEMM shape (M, N, K-slabs = K / 64) and epilogue class (1: BIAS_GEGLU), measured on MI355X (tools/time_linear.py
// --sweep, profiles/linear_sweep.md): the feed-forward and proj_out GEMMs of the SD1.5 UNet at 2 rows. Shapes not listed take the rule below.
struct LinTune { int M, N, nslab, geglu, bn, nsplit; };
constexpr LinTune LIN_TUNED[] = {
    // GEGLU projection (unsplit everywhere: N = 2 inner alone gives 320 - 2560 tiles)
    {8192, 2560, 5, 1, 64, 1}, {2048, 5120, 10, 1, 64, 1}, {512, 10240, 20, 1, 64, 1}, {128, 10240, 20, 1, 64, 1},
    // feed-forward output and proj_out (bias + residual)
    {8192, 320, 20, 0, 64, 1}, {8192, 320, 5, 0, 64, 1}, {2048, 640, 40, 0, 128, 3}, {2048, 640, 10, 0, 64, 1},
    {512, 1280, 80, 0, 64, 3}, {512, 1280, 20, 0, 64, 2}, {128, 1280, 80, 0, 64, 5}, {128, 1280, 20, 0, 64, 4},
};

struct LinPlan {
    int bn, nsplit, nslab, ntiles, nout;
    long xs, ys, rs;
};

bool plan_linear(const pww_linear_desc_t *d, LinPlan *p) {
    if (!d || d->size < sizeof(pww_linear_desc_t)) { set_error("linear: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return false; }
    const int e = d->epilogue;
    const bool geglu = e == PWW_LINEAR_BIAS_GEGLU;
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->M < 1 || d->K < 64 || d->K % 64 != 0 || d->N < 64 || d->N % 64 != 0
        || e < PWW_LINEAR_NONE || e > PWW_LINEAR_BIAS_GEGLU || (geglu && d->N % 128 != 0)) {
        set_error("linear: unsupported (dtype %d M %d N %d K %d epilogue %d): K and N multiples of 64, GEGLU's inner = N / 2 a multiple of 64", d->dtype,
                  d->M, d->N, d->K, e);
        return false;
    }
    p->nout = geglu ? d->N / 2 : d->N;
    p->xs = d->x_stride ? d->x_stride : d->K;
    p->ys = d->y_stride ? d->y_stride : p->nout;
    p->rs = d->r_stride ? d->r_stride : p->nout;
    if (p->xs < d->K || p->ys < p->nout || p->rs < p->nout || ((p->xs | p->ys | p->rs) & 7)) {
        set_error("linear: row strides must cover their rows and be multiples of 8 elements (x %ld y %ld r %ld)", p->xs, p->ys, p->rs);
        return false;
    }
    if ((long)d->M * p->xs >= (1L << 31) || (long)d->N * d->K >= (1L << 31) || (long)d->M * d->N >= (1L << 31)) { set_error("linear: tensor of 2^31 elements or more"); return false; }
    p->nslab = d->K / 64;
    const LinTune *tuned = nullptr;
    for (const LinTune &t : LIN_TUNED)
        if (t.M == d->M && t.N == d->N && t.nslab == p->nslab && t.geglu == (int)geglu) tuned = &t;
    p->bn = d->tile_n ? d->tile_n : tuned ? tuned->bn : (d->N % 128 == 0 ? 128 : 64);
    if ((p->bn != 64 && p->bn != 128) || d->N % p->bn != 0) { set_error("linear: tile_n %d does not divide N %d", d->tile_n, d->N); return false; }
    p->ntiles = (d->M + LN_BM - 1) / LN_BM * (d->N / p->bn);
    int ns = d->splitk;
    if (ns <= 0 && tuned && p->bn == tuned->bn) ns = tuned->nsplit;
    if (ns <= 0) {          // about 480 workgroups (2 per CU), at least 4 K-slabs per split
        ns = (480 + p->ntiles / 2) / p->ntiles;
        if (ns > p->nslab / 4) ns = p->nslab / 4;
        if (ns < 1) ns = 1;
    }
    if (ns > p->nslab || ns > 64) { set_error("linear: split %d exceeds the %d K-slabs (or 64)", ns, p->nslab); return false; }
    p->nsplit = ns;
    return true;
}

template <typename T>
int linear_launch(const LinPlan &p, const pww_linear_desc_t *d, const void *x, const void *w, const void *bias, const void *residual, void *y, void *ws,
                  hipStream_t stream) {
    LinCold cold{bias, residual, p.ys, p.rs, p.nsplit, p.nslab, d->epilogue, d->N / 2,
                 p.nsplit > 1 ? partial_stores_through((size_t)p.nsplit * d->M * d->N * sizeof(float)) : 0};
    const T *xt = static_cast<const T *>(x), *wt = static_cast<const T *>(w);
    const dim3 grid(p.ntiles * p.nsplit), block(LN_THREADS);
    void *out = p.nsplit == 1 ? y : ws;
    if (p.bn == 128) launch_timed(linear_kernel<T, 128>, grid, block, 0, stream, xt, wt, out, d->M, d->N, d->K, (int)p.xs, cold);
    else launch_timed(linear_kernel<T, 64>, grid, block, 0, stream, xt, wt, out, d->M, d->N, d->K, (int)p.xs, cold);
    if (p.nsplit == 1) return check_hip(hipGetLastError(), "linear launch");
    const long MN = (long)d->M * d->N, n4 = (long)d->M * p.nout / 4;
    launch_timed(linear_fold_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, static_cast<const float *>(ws), static_cast<T *>(y), n4,
                 d->N, MN, cold);
    return check_hip(hipGetLastError(), "linear fold launch");
}

bool al16(const void *a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace

size_t linear_workspace_bytes(const pww_linear_desc_t *d) {
    LinPlan p;
    if (!plan_linear(d, &p)) return 0;
    return p.nsplit > 1 ? (size_t)p.nsplit * d->M * d->N * sizeof(float) : 0;
}

int linear_fwd(const void *x, const void *w, const void *bias, const void *residual, void *y, const pww_linear_desc_t *d, void *workspace,
               size_t workspace_bytes, hipStream_t stream) {
    LinPlan p;
    if (!plan_linear(d, &p)) return PWW_ENOTSUP;
    if (!x || !w || !y) { set_error("linear: x, w and y are required"); return PWW_EINVAL; }
    if ((d->epilogue >= PWW_LINEAR_BIAS && !bias) || (d->epilogue == PWW_LINEAR_BIAS_RESIDUAL && !residual)) {
        set_error("linear: epilogue %d needs its bias%s", d->epilogue, d->epilogue == PWW_LINEAR_BIAS_RESIDUAL ? " and residual" : "");
        return PWW_EINVAL;
    }
    if (!al16(x) || !al16(w) || !al16(y) || (reinterpret_cast<uintptr_t>(bias) & 7) || (reinterpret_cast<uintptr_t>(residual) & 7)) {
        set_error("linear: x, w, y must be 16-byte aligned, bias and residual 8-byte aligned");
        return PWW_EINVAL;
    }
    const size_t need = p.nsplit > 1 ? (size_t)p.nsplit * d->M * d->N * sizeof(float) : 0;
    if (need && (!workspace || !al16(workspace) || workspace_bytes < need)) {
        set_error("linear: split %d needs a 16-byte aligned workspace of %zu bytes (got %zu)", p.nsplit, need, workspace_bytes);
        return PWW_EINVAL;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    if (d->dtype == PWW_DTYPE_F16) return linear_launch<f16>(p, d, x, w, bias, residual, y, workspace, stream);
    return linear_launch<bf16>(p, d, x, w, bias, residual, y, workspace, stream);
}

}  // namespace pww

PWW_LINEAR_API int pww_linear_version(void) { return PWW_LINEAR_VERSION; }
PWW_LINEAR_API const char *pww_linear_last_error(void) { return pww::last_error(); }
PWW_LINEAR_API size_t pww_linear_workspace_bytes(const pww_linear_desc_t *desc) { return pww::linear_workspace_bytes(desc); }
PWW_LINEAR_API int pww_linear_fwd(const void *x, const void *w, const void *bias, const void *residual, void *y, const pww_linear_desc_t *desc,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    return pww::linear_fwd(x, w, bias, residual, y, desc, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
