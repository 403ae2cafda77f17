// The residuals of a ControlNet on gfx950 MFMA as ONE grouped GEMM (pww_control_fwd): for every problem p of a table of at most 16,
//
//   out_p[m, c] = T(skip_p[m, c] + s * (sum_k h_p[m, k] * w_p[c, k] + b_p[c])),   s = scale_dev[scale_index] read by the kernel
//
// h_p [M, K] with a row stride (the [B H W, C] view of a channels_last hidden state), w_p [N, K] a 1 x 1 convolution's weight used in place,
// skip_p / out_p [M, N] with row strides (skip_p may be missing, out_p may alias it). One rounding, at the store. s == 0 hands the skip
// through bit for bit (zeros without one) whatever the accumulator holds: a select per element, so a ControlNet outside its guidance window
// cannot leak a NaN or flip the sign of a zero.
//
// The tile and the K loop are those of pww_linear.hip at its 64-wide tile: 128 (M) x 64 (N) x 64 (K) per 256-thread workgroup, 2 x 2 waves,
// mfma_f32_16x16x32 with the WEIGHT as the A operand (a lane holds 4 consecutive output channels of one row), LDS rows of 128 bytes with the
// 16-byte chunk index XOR-ed by (row & 7), CG_PF K-slabs of global loads in flight in register sets, a steady loop without conditions. The
// loop is WRITTEN AGAIN here, as pww_linear.hip wrote pww_conv.hip's again: sharing it through a header changed the register allocation
// and the wait counts of the convolution's code objects, and the measured times of both units rest on those. Nothing of libpww_hip_linear.so
// or of the convolutions is touched by this unit. The M tail loads from clamped rows and masks the store: no load sits under a condition.
//
// One launch: no split-K, no workspace, no atomics, no workgroup waits for another -- bitwise repeatable and legal under stream capture. The
// problem table travels BY VALUE in the kernel arguments (16 x 64 bytes + the prefix sums of the tile counts); a workgroup counts the prefix
// sums its id has passed (uniform, 15 scalar compares) and reads its problem's record with scalar loads. The host lays the table out in
// descending K (ties in the caller's order), so the tiles with the longest K loop are issued first and the short ones fill the tail.
//
// Built as a library of its own (libpww_hip_control.so, include/pww_hip_control.h): the unit is self-contained, its host plumbing is
// pww_side_host.h, and only the pww_control_* entry points are visible (compiled with -fvisibility=hidden).
#define PWW_SIDE_LIB "libpww_hip_control"
#include "pww_side_host.h"
#include "../../include/pww_hip_control.h"

#define PWW_CONTROL_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int CG_BM = PWW_CONTROL_TILE_M, CG_BN = PWW_CONTROL_TILE_N, CG_THREADS = 256, CG_MAX = PWW_CONTROL_MAX_PROBLEMS;
constexpr int CG_PF = 2;        // K-slabs of global loads in flight while one is computed (pww_linear.hip: LN_PF)

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// one problem as the kernel reads it (64 bytes: one 16-dword scalar load), and the table in issue order. first[q] = tiles in front of entry q;
// entries past n hold the launch's tile count, which no workgroup id reaches.
struct CgProblem {
    const void *h, *w, *bias, *skip;
    void *out;
    int M, N, K, hs, ss, os;
};
struct CgTable {
    CgProblem p[CG_MAX];
    int first[CG_MAX];
};

template <typename T>
__global__ void __launch_bounds__(CG_THREADS, 2) control_kernel(const float *__restrict__ scale_dev, int scale_index, const CgTable tab) {
    typedef typename Vec<T>::v8 V8;
    typedef typename Vec<T>::v4 V4;
    constexpr int BM = CG_BM, BN = CG_BN, PF = CG_PF, XL = BM * 8 / CG_THREADS, WL = BN * 8 / CG_THREADS, RM = 4, RN = BN / 32;
    constexpr int XBYTES = BM * 128, STAGE = (BM + BN) * 128;
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int bid = blockIdx.x;
    int q = 0;                                              // (uniform) the entry whose tiles hold this id
#pragma unroll
    for (int j = 1; j < CG_MAX; ++j) q += bid >= tab.first[j] ? 1 : 0;
    const CgProblem pr = tab.p[q];
    const int M = pr.M, K = pr.K;
    const int ntm = (M + BM - 1) / BM;
    const int tile = bid - tab.first[q];
    const int tm = tile % ntm, tn = tile / ntm;
    const T *x = static_cast<const T *>(pr.h), *w = static_cast<const T *>(pr.w);
    const float s = scale_dev[scale_index];

    // this thread's XL rows of h and WL rows of w (tile row (tid >> 3) + 32 i, 16-byte chunk tid & 7 of the slab)
    const int c = tid & 7;
    unsigned xoff[XL], woff[WL];
#pragma unroll
    for (int i = 0; i < XL; ++i) {
        int m = tm * BM + (tid >> 3) + 32 * i;
        m = m < M ? m : M - 1;
        xoff[i] = (unsigned)(m * pr.hs + c * 8);
    }
#pragma unroll
    for (int j = 0; j < WL; ++j) woff[j] = (unsigned)((tn * BN + (tid >> 3) + 32 * j) * K + c * 8);
    const int swz = ((c ^ ((tid >> 3) & 7)) << 4);          // LDS byte offset of this thread's chunk within its row

    // PF register sets, one K-slab of global loads each: set p holds slab i + p (mod PF) while slab i is computed
    u32x4 xr[PF][XL], wr[PF][WL];
    const T *xnext = x, *wnext = w;
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
            for (int u = 0; u < RM; ++u) {
                const int row = wm * 64 + u * 16 + fr;
                xf[u] = *reinterpret_cast<const V8 *>(bx + row * 128 + (((kk * 4 + fq) ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const int row = wn * (BN / 2) + r * 16 + fr;
                wf[r] = *reinterpret_cast<const V8 *>(bw + row * 128 + (((kk * 4 + fq) ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int r = 0; r < RN; ++r)
#pragma unroll
                for (int u = 0; u < RM; ++u) acc[r][u] = mfma16(wf[r], xf[u], acc[r][u]);
        }
    };

    // Slab i of the problem's n = K / 64 (>= 1) lives in register set i % PF until it moves to LDS buffer i & 1. Prologue: slabs 0 .. PF - 1
    // are requested, slab 0 lands in LDS (its wait counts past the younger sets' loads).
    const int n = K >> 6;
    load(0);
#pragma unroll
    for (int p = 1; p < PF; ++p)
        if (p < n) load(p);
    store(0, 0);
    __syncthreads();
    // Slab i: request slab i + PF into the set slab i came from, compute slab i from LDS, move slab i + 1 from its registers to the other
    // LDS buffer, one barrier. The steady loop is free of conditions, so the compiler's wait counts are exact.
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
    // drain: the last PF .. 2 PF - 1 slabs (or all of a short K), each request and move under its own condition
#pragma unroll
    for (int t = 0; t < 2 * PF - 1; ++t) {
        if (i + t < n) {
            if (i + t + PF < n) load(t % PF);
            compute((i + t) & 1);
            if (i + t + 1 < n) store((t + 1) % PF, (i + t + 1) & 1);
            __syncthreads();
        }
    }

    // lane holds D[tile column = wn BN / 2 + 16 r + 4 fq + j][m = 16 u + fr] of its wave's sub-tile: 4 consecutive channels of one row.
    // The skip is read by the thread that writes the same elements, so out may alias it.
    const T *bias = static_cast<const T *>(pr.bias), *skip = static_cast<const T *>(pr.skip);
    T *out = static_cast<T *>(pr.out);
    const bool off = s == 0.f;                              // (uniform)
#pragma unroll
    for (int u = 0; u < RM; ++u) {
        const int m = tm * BM + wm * 64 + u * 16 + fr;
        if (m >= M) continue;
#pragma unroll
        for (int r = 0; r < RN; ++r) {
            const int col = tn * BN + wn * (BN / 2) + r * 16 + fq * 4;
            const V4 b = *reinterpret_cast<const V4 *>(bias + col);
            V4 o;
            if (skip != nullptr) {                          // (uniform)
                const V4 k = *reinterpret_cast<const V4 *>(skip + (long)m * pr.ss + col);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = off ? k[j] : (T)((float)k[j] + s * (acc[r][u][j] + (float)b[j]));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = off ? (T)0.f : (T)(s * (acc[r][u][j] + (float)b[j]));
            }
            *reinterpret_cast<V4 *>(out + (long)m * pr.os + col) = o;
        }
    }
}

struct CgPlan {
    int order[CG_MAX];          // entry q of the table is the caller's problem order[q]
    int first[CG_MAX + 1];      // tiles in front of entry q; first[n] = the launch's tile count
    long hs[CG_MAX], ss[CG_MAX], os[CG_MAX];
};

// the shape half of the validation (what pww_control_plan and pww_control_fwd share): returns PWW_OK and fills the plan
int plan_control(const pww_control_problem_t *problems, int n, CgPlan *pl) {
    if (!problems) { set_error("control: the problem table is missing"); return PWW_EINVAL; }
    if (n < 1 || n > CG_MAX) { set_error("control: %d problems (1 .. %d)", n, CG_MAX); return PWW_EINVAL; }
    for (int p = 0; p < n; ++p) {
        const pww_control_problem_t &d = problems[p];
        if (d.M < 1 || d.K < 64 || d.K % 64 != 0 || d.N < 64 || d.N % 64 != 0) {
            set_error("control: problem %d unsupported (M %d N %d K %d): K and N multiples of 64, M >= 1", p, d.M, d.N, d.K);
            return PWW_ENOTSUP;
        }
        pl->hs[p] = d.h_stride ? d.h_stride : d.K;
        pl->ss[p] = d.skip_stride ? d.skip_stride : d.N;
        pl->os[p] = d.out_stride ? d.out_stride : d.N;
        if (pl->hs[p] < d.K || pl->ss[p] < d.N || pl->os[p] < d.N || ((pl->hs[p] | pl->ss[p] | pl->os[p]) & 7)) {
            set_error("control: problem %d: row strides must cover their rows and be multiples of 8 elements (h %ld skip %ld out %ld)", p, pl->hs[p], pl->ss[p],
                      pl->os[p]);
            return PWW_ENOTSUP;
        }
        if ((long)d.M * pl->hs[p] >= (1L << 31) || (long)d.N * d.K >= (1L << 31) || (long)d.M * pl->ss[p] >= (1L << 31) || (long)d.M * pl->os[p] >= (1L << 31)) {
            set_error("control: problem %d: tensor of 2^31 elements or more", p);
            return PWW_ENOTSUP;
        }
    }
    // descending K, ties in the caller's order (insertion sort: n <= 16)
    for (int p = 0; p < n; ++p) {
        int at = p;
        while (at > 0 && problems[pl->order[at - 1]].K < problems[p].K) { pl->order[at] = pl->order[at - 1]; --at; }
        pl->order[at] = p;
    }
    long total = 0;
    for (int q = 0; q < n; ++q) {
        const pww_control_problem_t &d = problems[pl->order[q]];
        pl->first[q] = (int)total;
        total += (long)((d.M + CG_BM - 1) / CG_BM) * (d.N / CG_BN);
        if (total >= (1L << 31)) { set_error("control: 2^31 tiles or more"); return PWW_ENOTSUP; }
    }
    pl->first[n] = (int)total;
    return PWW_OK;
}

template <typename T>
int control_launch(const CgTable &tab, int tiles, const float *scale_dev, int scale_index, hipStream_t stream) {
    launch_timed(control_kernel<T>, dim3((unsigned)tiles), dim3(CG_THREADS), 0, stream, scale_dev, scale_index, tab);
    return check_hip(hipGetLastError(), "control launch");
}

bool al(const void *a, unsigned mask) { return (reinterpret_cast<uintptr_t>(a) & mask) == 0; }

}  // namespace

int control_plan(const pww_control_problem_t *problems, int n, int32_t *out_tiles, int cap) {
    CgPlan pl;
    const int rc = plan_control(problems, n, &pl);
    if (rc != PWW_OK) return rc;
    if (cap < 0 || (cap > 0 && !out_tiles)) { set_error("control: plan needs room for its %d tiles", cap); return PWW_EINVAL; }
    int t = 0;
    for (int q = 0; q < n && t < cap; ++q) {
        const pww_control_problem_t &d = problems[pl.order[q]];
        const int ntm = (d.M + CG_BM - 1) / CG_BM, count = pl.first[q + 1] - pl.first[q];
        for (int tile = 0; tile < count && t < cap; ++tile, ++t) {       // (the kernel's decomposition of a workgroup id)
            out_tiles[3 * t] = pl.order[q];
            out_tiles[3 * t + 1] = (tile % ntm) * CG_BM;
            out_tiles[3 * t + 2] = (tile / ntm) * CG_BN;
        }
    }
    return pl.first[n];
}

int control_fwd(const pww_control_problem_t *problems, const pww_control_desc_t *d, const float *scale_dev, hipStream_t stream) {
    if (!d || d->size != sizeof(pww_control_desc_t)) { set_error("control: descriptor missing or of another ABI (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    if (d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) { set_error("control: dtype %d unsupported (float16 / bfloat16)", d->dtype); return PWW_ENOTSUP; }
    CgPlan pl;
    const int rc = plan_control(problems, d->n, &pl);
    if (rc != PWW_OK) return rc;
    if (!scale_dev || d->scale_index < 0 || !al(scale_dev, 3)) { set_error("control: the scale word is missing, misaligned or its index negative (%d)", d->scale_index); return PWW_EINVAL; }
    CgTable tab;
    memset(&tab, 0, sizeof(tab));
    for (int q = 0; q < CG_MAX; ++q) tab.first[q] = pl.first[q < d->n ? q : d->n];
    for (int q = 0; q < d->n; ++q) {
        const int p = pl.order[q];
        const pww_control_problem_t &s = problems[p];
        if (!s.h || !s.w || !s.bias || !s.out) { set_error("control: problem %d: h, w, bias and out are required", p); return PWW_EINVAL; }
        if (!al(s.h, 15) || !al(s.w, 15) || !al(s.out, 15) || !al(s.skip, 15) || !al(s.bias, 7)) {
            set_error("control: problem %d: h, w, skip, out must be 16-byte aligned, bias 8-byte aligned", p);
            return PWW_EINVAL;
        }
        tab.p[q] = CgProblem{s.h, s.w, s.bias, s.skip, s.out, s.M, s.N, s.K, (int)pl.hs[p], (int)pl.ss[p], (int)pl.os[p]};
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    if (d->dtype == PWW_DTYPE_F16) return control_launch<f16>(tab, pl.first[d->n], scale_dev, d->scale_index, stream);
    return control_launch<bf16>(tab, pl.first[d->n], scale_dev, d->scale_index, stream);
}

}  // namespace pww

PWW_CONTROL_API int pww_control_version(void) { return PWW_CONTROL_VERSION; }
PWW_CONTROL_API const char *pww_control_last_error(void) { return pww::last_error(); }
PWW_CONTROL_API int pww_control_plan(const pww_control_problem_t *problems, int32_t n, int32_t *out_tiles, int32_t cap) {
    return pww::control_plan(problems, n, out_tiles, cap);
}
PWW_CONTROL_API int pww_control_fwd(const pww_control_problem_t *problems, const pww_control_desc_t *desc, const float *scale_dev, void *stream) {
    return pww::control_fwd(problems, desc, scale_dev, static_cast<hipStream_t>(stream));
}
