// The second 3 x 3 convolution of a ResnetBlock2D that changes its channel count, with the block's 1 x 1 shortcut convolution as further
// K-slabs of the same implicit GEMM on gfx950 MFMA (pww_convtail_fwd):
//
//   y[m, n] = T( sum_k X[m, k] W[n, k]  +  sum_c X2[m, c] W2[n, c]  +  bias[n] + bias2[n] ),   m = (b, oy, ox),  k = (ky, kx, ci)
//
// The shortcut is a linear map summed into the same output, so the two sums are ONE GEMM with K' = 9 Cin + C2: the 1 x 1 convolution's own
// launch, the write of its output tensor and the epilogue's read of it as `residual` go away. K-slab s < 9 Cin / 64 is the gather of
// pww_conv.hip (stride 1, no upsample); a slab above that is the CENTRE tap of x2: no halo, row pitch C2, weight row `n C2` into w2. The
// source of a slab is chosen by wave-uniform selects of base pointer, pitch and tap -- never a branch around a load -- so the steady loop
// stays free of conditions and its waits stay counted.
//
// Tile, K loop, split-K with a fold launch, the XCD-aware tile order and the preloaded hot arguments are those of pww_conv.hip. The loop is
// WRITTEN AGAIN here (as in pww_linear.hip): a header shared with the convolution's unit changed the register allocation and the wait
// counts of its code objects, and those are what its measured times rest on. A split boundary may fall anywhere, inside the tail too.
//
// Epilogue (unsplit store and fold): T(acc + float(bias) + float(bias2)), ONE rounding; the unfused sequence rounds the shortcut, the
// convolution, the biased convolution and the sum.
//
// Built as a library of its own (libpww_hip_convtail.so, include/pww_hip_convtail.h): the unit is self-contained, its host plumbing is
// pww_side_host.h, and only the pww_convtail_* entry points are visible (compiled with -fvisibility=hidden).
#define PWW_SIDE_LIB "libpww_hip_convtail"
#include "pww_side_host.h"
#include "../../include/pww_hip_convtail.h"

#define PWW_CONVTAIL_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int CT_BM = 128, CT_THREADS = 256;
constexpr int CT_PF = 2;        // K-slabs of global loads in flight while one is computed (pww_conv.hip: CV_PF)

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// cold kernel arguments (behind the preloaded hot ones). nmain = 9 Cin / 64 slabs of the 3 x 3 gather, ntail = C2 / 64 of the shortcut
struct TailCold {
    const void *x2, *w2, *bias, *bias2;
    int nsplit, nmain, ntail;
    int through;            // split launches: the partials are stored write-through (pww_common.h: store_partial_through)
};

// bijective block-id remap: consecutive logical ids (tiles that share weight columns) on one XCD (guide T1)
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// T(acc + bias + bias2) of 4 consecutive channels n .. n + 3 at element offset off: one rounding
template <typename T>
__device__ __forceinline__ void epilogue4(const f32x4 &a, const TailCold &cold, T *y, long off, int n) {
    typedef typename Vec<T>::v4 V4;
    const V4 b = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias) + n);
    const V4 b2 = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias2) + n);
    V4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)(a[j] + (float)b[j] + (float)b2[j]);
    *reinterpret_cast<V4 *>(y + off) = o;
}

// Hot arguments first: 12 dwords preloaded into SGPRs.
template <typename T, int BN>
__global__ void __launch_bounds__(CT_THREADS, 2) convtail_kernel(const T *__restrict__ x, const T *__restrict__ w, void *__restrict__ out, int M, int N,
                                                                 int Cin, int C2, int H, int W, const TailCold cold) {
    typedef typename Vec<T>::v8 V8;
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
    const int K9 = 9 * Cin, HW = H * W;
    const T *__restrict__ x2 = reinterpret_cast<const T *>(cold.x2);
    const T *__restrict__ w2 = reinterpret_cast<const T *>(cold.w2);

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
    // this thread's weight row tn BN + (tid >> 3) (+ 32 j) in w (row pitch 9 Cin) and in w2 (row pitch C2), as element offsets
    const unsigned wrow = (unsigned)(tn * BN + (tid >> 3));
    const unsigned woff_main = wrow * (unsigned)K9 + c * 8, woff_tail = wrow * (unsigned)C2 + c * 8;
    const int swz = ((c ^ ((tid >> 3) & 7)) << 4);          // LDS byte offset of this thread's chunk within its row

    // PF register sets, one K-slab of global loads each: set p holds slab i + p (mod PF) while slab i is computed
    u32x4 xr[PF][XL], wr[PF][WL];
    unsigned xok[PF];
    // K position of the next slab: tap 0 .. 8 of the 3 x 3 gather, channel ci0 of it; tap 9 = the shortcut, ci0 its channel (never wraps)
    const bool tail0 = s_begin >= nmain;
    int tap = tail0 ? 9 : s_begin / (Cin >> 6);
    int ci0 = tail0 ? (s_begin - nmain) << 6 : (s_begin - tap * (Cin >> 6)) << 6;
    int kmain = s_begin * 64;                               // K offset into a row of w while the slab is one of the gather
    auto load = [&](int p) {                               // the next slab in K order into set p
        const bool tail = tap >= 9;                         // (uniform: selects of base, pitch and tap; every load below is issued)
        const int ky = tail ? 1 : tap / 3, kx = tail ? 1 : tap - (tap / 3) * 3;
        const T *xb = tail ? x2 : x;
        const T *wb = tail ? w2 : w;
        const int pitch = tail ? C2 : Cin;
        const unsigned wpitch = (unsigned)(tail ? C2 : K9);
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
template <typename T>
__global__ void __launch_bounds__(256) convtail_fold_kernel(const float *__restrict__ ws, T *__restrict__ y, long n4, int N, long MN, const TailCold cold) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    const long off = q * 4;
    f32x4 a = *reinterpret_cast<const f32x4 *>(ws + off);
    for (int s = 1; s < cold.nsplit; ++s) a += *reinterpret_cast<const f32x4 *>(ws + s * MN + off);
    epilogue4<T>(a, cold, y, off, (int)(off % N));
}

// Tile width and K split per shape (M = B H W, N = Cout, slabs of the gather, slabs of the shortcut), measured on MI355X
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

bool plan_tail(const pww_convtail_desc_t *d, TailPlan *p) {
    if (!d || d->size < sizeof(pww_convtail_desc_t)) { set_error("convtail: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return false; }
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 64 || d->Cin % 64 != 0 || d->C2 < 64
        || d->C2 % 64 != 0 || d->Cout < 64 || (d->Cout % 64 != 0 && d->Cout % 160 != 0) || d->Cin > 65536 || d->C2 > 65536 || d->Cout > 65536) {
        set_error("convtail: unsupported (dtype %d B %d %dx%d Cin %d C2 %d Cout %d): Cin and C2 multiples of 64, Cout of 64 or 160", d->dtype, d->B, d->H,
                  d->W, d->Cin, d->C2, d->Cout);
        return false;
    }
    const long M = (long)d->B * d->H * d->W;
    if (M * d->Cin >= (1L << 31) || M * d->C2 >= (1L << 31) || M * d->Cout >= (1L << 31) || 9L * d->Cin * d->Cout >= (1L << 31)
        || (long)d->C2 * d->Cout >= (1L << 31)) {
        set_error("convtail: tensor of 2^31 elements or more");
        return false;
    }
    p->M = (int)M;
    p->nmain = 9 * d->Cin / 64;
    p->ntail = d->C2 / 64;
    const int nslab = p->nmain + p->ntail;
    const TailTune *tuned = nullptr;
    for (const TailTune &t : TAIL_TUNED)
        if (t.M == p->M && t.N == d->Cout && t.nmain == p->nmain && t.ntail == p->ntail) tuned = &t;
    p->bn = d->tile_n ? d->tile_n : tuned ? tuned->bn : (d->Cout % 128 == 0 ? 128 : d->Cout % 64 == 0 ? 64 : 160);
    if ((p->bn != 64 && p->bn != 128 && p->bn != 160) || d->Cout % p->bn != 0) { set_error("convtail: tile_n %d does not divide Cout %d", d->tile_n, d->Cout); return false; }
    p->ntiles = (p->M + CT_BM - 1) / CT_BM * (d->Cout / p->bn);
    int ns = d->splitk;
    if (ns <= 0 && tuned && p->bn == tuned->bn) ns = tuned->nsplit;
    if (ns <= 0) {          // about 480 workgroups (2 per CU), at least 8 K-slabs per split
        ns = (480 + p->ntiles / 2) / p->ntiles;
        if (ns > nslab / 8) ns = nslab / 8;
        if (ns < 1) ns = 1;
    }
    if (ns > nslab || ns > 64) { set_error("convtail: split %d exceeds the %d K-slabs (or 64)", ns, nslab); return false; }
    p->nsplit = ns;
    return true;
}

template <typename T>
int tail_launch(const TailPlan &p, const pww_convtail_desc_t *d, const void *x, const void *w, const void *x2, const void *w2, const void *bias,
                const void *bias2, void *y, void *ws, hipStream_t stream) {
    const int N = d->Cout;
    TailCold cold{x2, w2, bias, bias2, p.nsplit, p.nmain, p.ntail, p.nsplit > 1 ? partial_stores_through((size_t)p.nsplit * p.M * N * sizeof(float)) : 0};
    const T *xt = static_cast<const T *>(x), *wt = static_cast<const T *>(w);
    const dim3 grid(p.ntiles * p.nsplit), block(CT_THREADS);
    void *out = p.nsplit == 1 ? y : ws;
    if (p.bn == 160) {
        constexpr size_t lds = 2 * (CT_BM + 160) * 128;
        static thread_local LdsRaised raised;       // (of convtail_kernel<T, 160>: this function is instantiated per T)
        if (raise_lds_limit(convtail_kernel<T, 160>, lds, raised)) return PWW_EHIP;
        launch_timed(convtail_kernel<T, 160>, grid, block, lds, stream, xt, wt, out, p.M, N, d->Cin, d->C2, d->H, d->W, cold);
    } else if (p.bn == 128) launch_timed(convtail_kernel<T, 128>, grid, block, 0, stream, xt, wt, out, p.M, N, d->Cin, d->C2, d->H, d->W, cold);
    else launch_timed(convtail_kernel<T, 64>, grid, block, 0, stream, xt, wt, out, p.M, N, d->Cin, d->C2, d->H, d->W, cold);
    if (p.nsplit == 1) return check_hip(hipGetLastError(), "convtail launch");
    const long MN = (long)p.M * N, n4 = MN / 4;
    launch_timed(convtail_fold_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, static_cast<const float *>(ws), static_cast<T *>(y), n4,
                 N, MN, cold);
    return check_hip(hipGetLastError(), "convtail fold launch");
}

}  // namespace

size_t convtail_workspace_bytes(const pww_convtail_desc_t *d) {
    TailPlan p;
    if (!plan_tail(d, &p)) return 0;
    return p.nsplit > 1 ? (size_t)p.nsplit * p.M * d->Cout * sizeof(float) : 0;
}

int convtail_fwd(const void *x, const void *w, const void *x2, const void *w2, const void *bias, const void *bias2, void *y, const pww_convtail_desc_t *d,
                 void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!d || d->size < sizeof(pww_convtail_desc_t)) { set_error("convtail: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    TailPlan p;
    if (!plan_tail(d, &p)) return PWW_ENOTSUP;
    if (!x || !w || !x2 || !w2 || !bias || !bias2 || !y) { set_error("convtail: x, w, x2, w2, bias, bias2 and y are required"); return PWW_EINVAL; }
    if (!aligned16(x) || !aligned16(w) || !aligned16(x2) || !aligned16(w2) || !aligned16(y) || (reinterpret_cast<uintptr_t>(bias) & 7)
        || (reinterpret_cast<uintptr_t>(bias2) & 7)) {
        set_error("convtail: x, w, x2, w2, y must be 16-byte aligned, the biases 8-byte aligned");
        return PWW_EINVAL;
    }
    const size_t need = p.nsplit > 1 ? (size_t)p.nsplit * p.M * d->Cout * sizeof(float) : 0;
    if (need && (!workspace || !aligned16(workspace) || workspace_bytes < need)) {
        set_error("convtail: split %d needs a 16-byte aligned workspace of %zu bytes (got %zu)", p.nsplit, need, workspace_bytes);
        return PWW_EINVAL;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    if (d->dtype == PWW_DTYPE_F16) return tail_launch<f16>(p, d, x, w, x2, w2, bias, bias2, y, workspace, stream);
    return tail_launch<bf16>(p, d, x, w, x2, w2, bias, bias2, y, workspace, stream);
}

}  // namespace pww

PWW_CONVTAIL_API int pww_convtail_version(void) { return PWW_CONVTAIL_VERSION; }
PWW_CONVTAIL_API const char *pww_convtail_last_error(void) { return pww::last_error(); }
PWW_CONVTAIL_API size_t pww_convtail_workspace_bytes(const pww_convtail_desc_t *desc) { return pww::convtail_workspace_bytes(desc); }
PWW_CONVTAIL_API int pww_convtail_fwd(const void *x, const void *w, const void *x2, const void *w2, const void *bias, const void *bias2, void *y,
                                      const pww_convtail_desc_t *desc, void *workspace, size_t workspace_bytes, void *stream) {
    return pww::convtail_fwd(x, w, x2, w2, bias, bias2, y, desc, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
