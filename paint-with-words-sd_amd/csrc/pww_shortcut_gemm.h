// conv2 of a ResnetBlock2D with the block's 1 x 1 shortcut as further K-slabs of the same implicit GEMM on gfx950 MFMA: the ONE source of
// the kernel, its fold, its measured plans and its launch, for the two units that instantiate it --
//
//   pww_conv_tail.hip   (libpww_hip_convtail.so)   shortcut_gemm_kernel<T, BN, TailCold, int>          the shortcut's input is one tensor
//   pww_concat.hip      (libpww_hip_concat.so)     shortcut_gemm_kernel<T, BN, CatTailCold, int, int>  ... two tensors, read where they lie
//
//   y[m, n] = T( sum_k X[m, k] W[n, k]  +  sum_c X2[m, c] W2[n, c]  +  bias[n] + bias2[n] ),   m = (b, oy, ox),  k = (ky, kx, ci)
//
// K-slab s < 9 Cin / 64 is the gather of pww_conv.hip (stride 1, no upsample); a slab above that is the CENTRE tap of the shortcut's
// input: no halo, row pitch of its source, weight row `n Ct` into wsc. The source of a slab is chosen by wave-uniform selects of base
// pointer, pitch and tap -- never a branch around a load -- so the steady loop stays free of conditions and its waits stay counted. With
// two sources, tail slab t reads x1 (pitch C1) while 64 t < C1, then x2 (pitch C2, channel 64 t - C1). A split boundary may fall anywhere,
// inside the tail too.
//
// Tile, K loop, split-K with a fold launch, the XCD-aware tile order and the preloaded hot arguments are those of pww_conv.hip. The loop
// is written again here and not shared with THAT unit (as in pww_linear.hip): a header shared with it changed the register allocation
// and the wait counts of its code objects, and those are what its measured times rest on. Between the two units above the kernel IS
// shared, as what it is, a `__global__` template: their sixteen code objects are instruction for instruction those of the two written-out
// copies this header replaces. A shared `__device__ __forceinline__` body behind thin `__global__` wrappers is not: over one common
// argument list it moved the register allocation of all twelve main code objects, and even forwarded pack for pack it comes out with
// other operand orders (profiles/shortcut_gemm.md). Keep the kernel a template of `Parts...`: the pack is the hot argument list's only
// difference, so each unit keeps its kernarg layout and its 12 / 13 preloaded dwords.
//
// Epilogue (unsplit store and fold): T(acc + float(bias) + float(bias2)), ONE rounding; the unfused sequence rounds the shortcut, the
// convolution, the biased convolution and the sum.
//
// Included once by each unit, at file scope, after pww_side_host.h. A unit's cold struct carries x1 (and x2 with two sources), wsc, bias,
// bias2, then the ints nsplit, nmain, ntail, through; the unit fills the pointers, the launch below the rest.
#pragma once
#include "pww_common.h"

namespace pww {

namespace {

constexpr int CT_BM = 128, CT_THREADS = 256;
constexpr int CT_PF = 2;        // K-slabs of global loads in flight while one is computed (pww_conv.hip: CV_PF)

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// bijective block-id remap: consecutive logical ids (tiles that share weight columns) on one XCD (guide T1)
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// T(acc + bias + bias2) of 4 consecutive channels n .. n + 3 at element offset off: one rounding
template <typename T, typename Cold>
__device__ __forceinline__ void epilogue4(const f32x4 &a, const Cold &cold, T *y, long off, int n) {
    typedef typename Vec<T>::v4 V4;
    const V4 b = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias) + n);
    const V4 b2 = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias2) + n);
    V4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)(a[j] + (float)b[j] + (float)b2[j]);
    *reinterpret_cast<V4 *>(y + off) = o;
}

// Hot arguments first: 12 dwords (one source: parts = C1) or 13 (two: C1, C2) preloaded into SGPRs. The cold struct follows: the shortcut's
// pointers are first needed after 9 Cin / 64 slabs (or at once in a split that starts in the tail, whose prologue waits for the cold
// struct anyway for nsplit). nmain = 9 Cin / 64 slabs of the 3 x 3 gather, ntail = Ct / 64 of the shortcut.
template <typename T, int BN, typename Cold, typename... Parts>
__global__ void __launch_bounds__(CT_THREADS, 2) shortcut_gemm_kernel(const T *__restrict__ x, const T *__restrict__ w, void *__restrict__ out, int M, int N,
                                                                      int Cin, Parts... parts, int H, int W, const Cold cold) {
    typedef typename Vec<T>::v8 V8;
    constexpr bool TWO = sizeof...(Parts) == 2;
    static_assert(sizeof...(Parts) == 1 || TWO, "parts: C1, or C1 and C2");
    constexpr int BM = CT_BM, PF = CT_PF, XL = BM * 8 / CT_THREADS, WL = BN * 8 / CT_THREADS, RM = 4, RN = BN / 32;
    constexpr int XBYTES = BM * 128, STAGE = (BM + BN) * 128;
    // two stages: a static array, or above 64 KB (the 160-wide tile: 73 728 bytes) the launch-sized one (pww_conv.hip)
    constexpr bool DYN = 2 * STAGE > 64 * 1024;
    __shared__ __attribute__((aligned(16))) char lds[DYN ? 16 : 2 * STAGE];
    auto stage = [&](int buf) -> char * {
        if constexpr (DYN) return launch_lds() + buf * STAGE;
        else return lds + buf * STAGE;
    };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int ntm = (M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const bool split = cold.nsplit > 1;                     // (uniform: one code object serves both, the partial store is its only other trace)
    const int tile = bid / cold.nsplit, ks = bid - tile * cold.nsplit;
    const int tm = tile % ntm, tn = tile / ntm;
    const int nmain = cold.nmain, nslab = nmain + cold.ntail;
    const int s_begin = (int)((long)ks * nslab / cold.nsplit), s_end = (int)((long)(ks + 1) * nslab / cold.nsplit);
    const int part[] = {parts...};
    const int C1 = part[0], C2 = part[sizeof...(Parts) - 1];
    const int K9 = 9 * Cin, HW = H * W, Ct = TWO ? C1 + C2 : C1;
    const T *__restrict__ xa = reinterpret_cast<const T *>(cold.x1);
    const T *__restrict__ xb2 = nullptr;
    if constexpr (TWO) xb2 = reinterpret_cast<const T *>(cold.x2);
    const T *__restrict__ w2 = reinterpret_cast<const T *>(cold.wsc);

    // the gather geometry of this thread's XL rows (row (tid >> 3) + 32 i, 16-byte chunk tid & 7 of the slab)
    const int c = tid & 7;
    int pix[XL], y0[XL], x0[XL];
#pragma unroll
    for (int i = 0; i < XL; ++i) {
        int m = tm * BM + (tid >> 3) + 32 * i;
        m = m < M ? m : M - 1;
        const int b = m / HW, rem = m - b * HW, oy = rem / W, ox = rem - oy * W;
        pix[i] = b * HW;
        y0[i] = oy - 1;
        x0[i] = ox - 1;
    }
    // this thread's weight row tn BN + (tid >> 3) (+ 32 j) in w (row pitch 9 Cin) and in wsc (row pitch Ct), as element offsets
    const unsigned wrow = (unsigned)(tn * BN + (tid >> 3));
    const unsigned woff_main = wrow * (unsigned)K9 + c * 8, woff_tail = wrow * (unsigned)Ct + c * 8;
    const int swz = ((c ^ ((tid >> 3) & 7)) << 4);          // LDS byte offset of this thread's chunk within its row

    // PF register sets, one K-slab of global loads each: set p holds slab i + p (mod PF) while slab i is computed
    u32x4 xr[PF][XL], wr[PF][WL];
    unsigned xok[PF];
    // K position of the next slab: tap 0 .. 8 of the 3 x 3 gather, channel ci0 of it; tap 9 = the shortcut, ci0 its channel in the (one
    // tensor or concatenation of two) shortcut input (never wraps)
    const bool tail0 = s_begin >= nmain;
    int tap = tail0 ? 9 : s_begin / (Cin >> 6);
    int ci0 = tail0 ? (s_begin - nmain) << 6 : (s_begin - tap * (Cin >> 6)) << 6;
    int kmain = s_begin * 64;                               // K offset into a row of w while the slab is one of the gather
    // the tail slab's source: x1 while ci0 < C1, then x2 with its channel origin folded into the pointer (x2 - C1: only ever dereferenced
    // at ci0 >= C1), so that a tail address is `base + pixel * pitch + ci0` for both; switched by a select when ci0 reaches C1
    const bool second0 = TWO && tail0 && ci0 >= C1;
    const T *xs = second0 ? xb2 - C1 : xa;
    int ps = second0 ? C2 : C1;
    auto load = [&](int p) {                               // the next slab in K order into set p
        const bool tail = tap >= 9;                         // (uniform: selects of base, pitch and tap; every load below is issued)
        const int ky = tail ? 1 : tap / 3, kx = tail ? 1 : tap - (tap / 3) * 3;
        const T *xb = tail ? xs : x;
        const T *wb = tail ? w2 : w;
        const int pitch = tail ? ps : Cin;
        const unsigned wpitch = (unsigned)(tail ? Ct : K9);
        const unsigned wo = (tail ? woff_tail : woff_main) + (unsigned)(tail ? ci0 : kmain);
        xok[p] = 0;
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int iy = y0[i] + ky, ix = x0[i] + kx;
            const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;     // (the centre tap is always inside)
            xr[p][i] = *reinterpret_cast<const u32x4 *>(xb + (unsigned)((pix[i] + (ok ? iy : 0) * W + (ok ? ix : 0)) * pitch + ci0 + c * 8));
            xok[p] |= (unsigned)ok << i;
        }
#pragma unroll
        for (int j = 0; j < WL; ++j) wr[p][j] = *reinterpret_cast<const u32x4 *>(wb + (wo + (unsigned)(32 * j) * wpitch));
        kmain += 64;
        ci0 += 64;
        const bool wrap = ci0 == Cin && !tail;              // (the last tap wraps into the tail: tap 9, channel 0)
        ci0 = wrap ? 0 : ci0;
        tap += wrap ? 1 : 0;
        if constexpr (TWO) {
            const bool cross = ci0 == C1 && tail;           // (uniform: the next tail slab is the first of x2)
            xs = cross ? xb2 - C1 : xs;
            ps = cross ? C2 : ps;
        }
    };
    auto store = [&](int p, int buf) {
        char *base = stage(buf);
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const u32x4 z = {0u, 0u, 0u, 0u};           // (the halo's select sits here, after the compute: the loads stay in flight across it)
            *reinterpret_cast<u32x4 *>(base + ((tid >> 3) + 32 * i) * 128 + swz) = (xok[p] >> i) & 1u ? xr[p][i] : z;
        }
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
        const char *bx = stage(buf), *bw = bx + XBYTES;
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
            __builtin_amdgcn_sched_barrier(0);              // (the halo's select stays behind the compute: hoisted to the loop's head it waits for every load in flight)
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

    // lane holds D[n = 16 r + 4 fq + j][m = 16 i + fr] of its wave's sub-tile
    if (split && cold.through) {                            // (uniform) the partials written through: pww_common.h, store_partial_through
        const unsigned ws_bytes = (unsigned)cold.nsplit * (unsigned)M * (unsigned)N * 4u;      // (the host asks for this only below 4 GiB)
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            const int m = tm * BM + wm * 64 + i * 16 + fr;
            if (m >= M) continue;
#pragma unroll
            for (int r = 0; r < RN; ++r) {
                const int n = tn * BN + wn * (BN / 2) + r * 16 + fq * 4;
                store_partial_through(out, ws_bytes, (((unsigned)ks * (unsigned)M + (unsigned)m) * (unsigned)N + (unsigned)n) * 4u, acc[r][i]);
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < RM; ++i) {
        const int m = tm * BM + wm * 64 + i * 16 + fr;
        if (m >= M) continue;
#pragma unroll
        for (int r = 0; r < RN; ++r) {
            const int n = tn * BN + wn * (BN / 2) + r * 16 + fq * 4;
            if (split) *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(out) + ((long)ks * M + m) * N + n) = acc[r][i];
            else epilogue4<T>(acc[r][i], cold, reinterpret_cast<T *>(out), (long)m * N + n, n);
        }
    }
}

// fold the split-K partials [nsplit][M][N] in split order, then the epilogue: one thread per 4 channels of one pixel
template <typename T, typename Cold>
__global__ void __launch_bounds__(256) shortcut_fold_kernel(const float *__restrict__ ws, T *__restrict__ y, long n4, int N, long MN, const Cold cold) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    const long off = q * 4;
    f32x4 a = *reinterpret_cast<const f32x4 *>(ws + off);
    for (int s = 1; s < cold.nsplit; ++s) a += *reinterpret_cast<const f32x4 *>(ws + s * MN + off);
    epilogue4<T>(a, cold, y, off, (int)(off % N));
}

// Tile width and K split per shape (M = B H W, N = Cout, slabs of the gather, slabs of the shortcut = Ct / 64), measured on MI355X
// (tools/time_convtail.py --sweep, profiles/conv_shortcut.md): the fourteen channel-changing ResnetBlock2D of the SD1.5 UNet at 2 rows.
// Shapes not listed take the rule of pww_conv.hip (about 480 workgroups, at least 8 K-slabs per split).
struct TailTune { int M, N, nmain, ntail, bn, nsplit; };
constexpr TailTune TAIL_TUNED[] = {
    {128, 1280, 180, 40, 64, 12},
    {512, 1280, 180, 40, 128, 12}, {512, 1280, 180, 30, 128, 12}, {512, 1280, 180, 10, 128, 12},
    {2048, 640, 90, 30, 128, 6}, {2048, 640, 90, 20, 128, 6}, {2048, 640, 90, 15, 128, 6}, {2048, 640, 90, 5, 128, 6},
    {8192, 320, 45, 15, 160, 4}, {8192, 320, 45, 10, 160, 4},        // (profiles/conv_wide160.md: 46.2 -> 39.7 and 43.8 -> 38.2 us)
};

struct TailPlan {
    int M, bn, nsplit, nmain, ntail, ntiles;
};

// Tile width, tile count and K split of a validated shape; `what` names the entry point in the two refusals that are the plan's own
bool plan_tail(const char *what, int M, int nmain, int ntail, int Cout, int tile_n, int splitk, TailPlan *p) {
    p->M = M;
    p->nmain = nmain;
    p->ntail = ntail;
    const int nslab = nmain + ntail;
    const TailTune *tuned = nullptr;
    for (const TailTune &t : TAIL_TUNED)
        if (t.M == M && t.N == Cout && t.nmain == nmain && t.ntail == ntail) tuned = &t;
    p->bn = tile_n ? tile_n : tuned ? tuned->bn : (Cout % 128 == 0 ? 128 : Cout % 64 == 0 ? 64 : 160);
    if ((p->bn != 64 && p->bn != 128 && p->bn != 160) || Cout % p->bn != 0) { set_error("%s: tile_n %d does not divide Cout %d", what, tile_n, Cout); return false; }
    p->ntiles = (M + CT_BM - 1) / CT_BM * (Cout / p->bn);
    int ns = splitk;
    if (ns <= 0 && tuned && p->bn == tuned->bn) ns = tuned->nsplit;
    if (ns <= 0) {          // about 480 workgroups (2 per CU), at least 8 K-slabs per split
        ns = (480 + p->ntiles / 2) / p->ntiles;
        if (ns > nslab / 8) ns = nslab / 8;
        if (ns < 1) ns = 1;
    }
    if (ns > nslab || ns > 64) { set_error("%s: split %d exceeds the %d K-slabs (or 64)", what, ns, nslab); return false; }
    p->nsplit = ns;
    return true;
}

// the fp32 partials [nsplit][M][Cout] of a split plan; 0: no workspace
size_t tail_workspace_bytes(const TailPlan &p, int Cout) { return p.nsplit > 1 ? (size_t)p.nsplit * p.M * Cout * sizeof(float) : 0; }

// The main launch at the plan's tile width and, for a split plan, the fold. `cold` arrives with its pointers; `parts` is C1 or C1, C2.
template <typename T, typename Cold, typename... Parts>
int tail_launch(const char *what, const TailPlan &p, const void *x, const void *w, Cold cold, void *y, void *ws, int N, int Cin, int H, int W,
                hipStream_t stream, Parts... parts) {
    cold.nsplit = p.nsplit;
    cold.nmain = p.nmain;
    cold.ntail = p.ntail;
    cold.through = p.nsplit > 1 ? partial_stores_through(tail_workspace_bytes(p, N)) : 0;
    const T *xt = static_cast<const T *>(x), *wt = static_cast<const T *>(w);
    const dim3 grid(p.ntiles * p.nsplit), block(CT_THREADS);
    void *out = p.nsplit == 1 ? y : ws;
    if (p.bn == 160) {
        constexpr size_t lds = 2 * (CT_BM + 160) * 128;
        static thread_local LdsRaised raised;       // (of the 160-wide kernel of this T and unit: the function is instantiated per both)
        if (raise_lds_limit(shortcut_gemm_kernel<T, 160, Cold, Parts...>, lds, raised)) return PWW_EHIP;
        launch_timed(shortcut_gemm_kernel<T, 160, Cold, Parts...>, grid, block, lds, stream, xt, wt, out, p.M, N, Cin, parts..., H, W, cold);
    } else if (p.bn == 128) launch_timed(shortcut_gemm_kernel<T, 128, Cold, Parts...>, grid, block, 0, stream, xt, wt, out, p.M, N, Cin, parts..., H, W, cold);
    else launch_timed(shortcut_gemm_kernel<T, 64, Cold, Parts...>, grid, block, 0, stream, xt, wt, out, p.M, N, Cin, parts..., H, W, cold);
    char step[48];
    snprintf(step, sizeof(step), "%s%s launch", what, p.nsplit == 1 ? "" : " fold");
    if (p.nsplit == 1) return check_hip(hipGetLastError(), step);
    const long MN = (long)p.M * N, n4 = MN / 4;
    launch_timed(shortcut_fold_kernel<T, Cold>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, static_cast<const float *>(ws), static_cast<T *>(y), n4,
                 N, MN, cold);
    return check_hip(hipGetLastError(), step);
}

}  // namespace

}  // namespace pww
