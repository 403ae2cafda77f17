// 3 x 3 convolution (padding 1) over NHWC tensors as an implicit GEMM on gfx950 MFMA (pww_conv3x3_fwd):
//
//   y[m, n] = sum_k X[m, k] * W[n, k],   m = (b, oy, ox),  n = output channel,  k = (ky, kx, ci)
//
// K is ordered (ky, kx, ci), the layout of a channels_last nn.Conv2d weight ([Cout][3][3][Cin]), so one K-slab of 64 is a contiguous run of
// 64 channels of ONE tap: 16-byte loads straight from the activation for X and from the weight row for W. The padding halo (and the
// M tail) loads from a clamped address and selects zero after the load -- no branch around a load. Stride 2 (Downsample2D) and a
// nearest 2x upsample of the input (Upsample2D: the gather reads x[iy >> 1][ix >> 1]) are index arithmetic of the same gather.
//
// Tile: 128 (M) x BN (N, 64 or 128) x 64 (K) per 256-thread workgroup, 2 x 2 waves, mfma_f32_16x16x32 with the WEIGHT as the A operand:
// the accumulator then holds 4 consecutive channels of one pixel per lane (8-byte stores, 8-byte bias / residual loads). LDS rows of 128
// bytes with the 16-byte chunk index XOR-ed by (row & 7).
//
// K loop: CV_PF K-slabs of global loads are in flight while a slab is computed. Slab i waits in register set i % CV_PF and moves to LDS
// buffer i & 1 (two buffers) after slab i - 1 has been computed, one barrier per slab; the set is requested again (slab i + CV_PF) right
// after that barrier. The wait ahead of the move is counted (vmcnt = the loads of the CV_PF - 1 younger slabs), never a drain, and the loads
// stay in flight across the barrier. The steady loop is unrolled CV_PF times and holds no condition, so that the compiler's counts are
// exact; the last slabs (and splits shorter than 2 CV_PF slabs) go through a drain whose requests and moves are conditional.
//
// Split-K (the 16 x 16 and 8 x 8 levels have too few tiles for 256 CUs): each workgroup writes its fp32 partial tile to a caller-owned
// workspace, a second launch folds the partials in fixed order and applies the epilogue. No atomics, no inter-workgroup waits: results
// are bitwise repeatable.
//
// Epilogue, with the stock sequence's rounding points (T = storage type):  v = T(acc);  v = T(v + bias[n]) (bias);  v = T(residual + v)
// (residual) -- exactly what conv -> pww_bias_residual computed.
#include "pww_common.h"

namespace pww {

namespace {

constexpr int CV_BM = 128, CV_THREADS = 256;
// K-slabs of global loads in flight while one slab is computed. 2 measured 2 - 10 % faster than 1 on every UNet shape at 2 rows; 3 costs
// 252 VGPRs at BN 128 and the third workgroup per CU at BN 64 and measured no better than 1 (profiles/conv3x3_pipeline.md).
constexpr int CV_PF = 2;

// This file is compiled twice. As a unit of libpww_hip.so it instantiates the 64- and 128-wide tiles. The 160-wide tile's two code objects
// do not fit under that library's size limit: pww_convwide.hip includes this file with PWW_CONV_WIDE_UNIT defined and libpww_hip_convwide.so
// carries them (pww_convwide_*), with the same plan and table -- one source, so the two libraries cannot disagree about a shape.
// A third compile, pww_vaeenc.hip with PWW_CONV_DOWN_UNIT defined, is the AutoencoderKL encoder's downsampler (libpww_hip_vaeenc.so,
// pww_vaeenc_down_*): stride 2 with the zero padding on the right and bottom only, i.e. the pad origin at 0 and Ho = (H - 2) / 2 + 1, on
// the 64- and 128-wide tiles. With neither macro defined the file expands to exactly what it was before that unit existed.
__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// cold kernel arguments (behind the preloaded hot ones)
struct ConvCold {
    const void *bias, *residual;
    int nsplit, nslab;
    int through;            // split launches: the partials are stored write-through (pww_common.h: store_partial_through)
};

// bijective block-id remap: consecutive logical ids (tiles that share weight columns) on one XCD (guide T1)
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

template <typename T>
__device__ __forceinline__ void epilogue4(const f32x4 &a, const ConvCold &cold, T *y, long off, int n) {
    typedef typename Vec<T>::v4 V4;
    V4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)a[j];
    if (cold.bias) {
        const V4 b = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias) + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (T)((float)o[j] + (float)b[j]);
    }
    if (cold.residual) {
        const V4 r = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.residual) + off);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (T)((float)r[j] + (float)o[j]);
    }
    *reinterpret_cast<V4 *>(y + off) = o;
}

// geo = stride | (upsample << 4). Hot arguments first: 14 dwords preloaded into SGPRs.
template <typename T, int BN>
__global__ void __launch_bounds__(CV_THREADS, 2) conv3x3_kernel(const T *__restrict__ x, const T *__restrict__ w, void *__restrict__ out, int M, int N,
                                                            int Cin, int Hin, int Win, int Wo, int HWo, const ConvCold cold) {
    typedef typename Vec<T>::v8 V8;
    constexpr int BM = CV_BM, PF = CV_PF, XL = BM * 8 / CV_THREADS, WL = BN * 8 / CV_THREADS, RM = 4, RN = BN / 32;
    constexpr int XBYTES = BM * 128, STAGE = (BM + BN) * 128;
    // two stages: a static array, or above 64 KB (the 160-wide tile: 73 728 bytes) the launch-sized one, as in the attention kernels. The
    // narrower instantiations keep the array itself in every expression -- through a pointer their register allocation moved
    constexpr bool DYN = 2 * STAGE > 64 * 1024;
    __shared__ __attribute__((aligned(16))) char lds[DYN ? 16 : 2 * STAGE];
    auto stage = [&](int buf) -> char * {
        if constexpr (DYN) return launch_lds() + buf * STAGE;
        else return lds + buf * STAGE;
    };

    const int geo = cold.nslab >> 24;                       // (packed by the host: stride | upsample << 4)
    const int nslab = cold.nslab & 0xffffff;
    const int stride = geo & 15, up = geo >> 4;
    const int Hv = Hin << up, Wv = Win << up;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int ntm = (M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const bool split = cold.nsplit > 1;                     // (uniform: one code object serves both, the partial store is its only other trace)
    const int tile = bid / cold.nsplit, ks = bid - tile * cold.nsplit;
    const int tm = tile % ntm, tn = tile / ntm;
    const int s_begin = (int)((long)ks * nslab / cold.nsplit), s_end = (int)((long)(ks + 1) * nslab / cold.nsplit);
    const int K9 = 9 * Cin;

    // the gather geometry of this thread's XL rows (row (tid >> 3) + 32 i, 16-byte chunk tid & 7 of the slab)
    const int c = tid & 7;
    int pix[XL], y0[XL], x0[XL];
#pragma unroll
    for (int i = 0; i < XL; ++i) {
        int m = tm * BM + (tid >> 3) + 32 * i;
        m = m < M ? m : M - 1;
        const int b = m / HWo, rem = m - b * HWo, oy = rem / Wo, ox = rem - oy * Wo;
        pix[i] = b * Hin * Win;
#ifdef PWW_CONV_DOWN_UNIT
        y0[i] = oy * stride;        // no padding on the top and left: the taps are rows 2 oy + {0, 1, 2} (the halo test below covers the bottom and right)
        x0[i] = ox * stride;
#else
        y0[i] = oy * stride - 1;
        x0[i] = ox * stride - 1;
#endif
    }
    const T *wrow = w + (long)(tn * BN + (tid >> 3)) * K9 + c * 8;
    const int swz = ((c ^ ((tid >> 3) & 7)) << 4);          // LDS byte offset of this thread's chunk within its row

    // PF register sets, one K-slab of global loads each: set p holds slab i + p (mod PF) while slab i is computed
    u32x4 xr[PF][XL], wr[PF][WL];
    unsigned xok[PF];
    int tap = s_begin / (Cin >> 6), ci0 = (s_begin - tap * (Cin >> 6)) << 6;
    const T *wnext = wrow + s_begin * 64;
    auto load = [&](int p) {                               // the next slab in K order into set p
        const int ky = tap / 3, kx = tap - ky * 3;
        xok[p] = 0;
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int iyv = y0[i] + ky, ixv = x0[i] + kx;
            const bool ok = (unsigned)iyv < (unsigned)Hv && (unsigned)ixv < (unsigned)Wv;
            const int iy = ok ? iyv >> up : 0, ix = ok ? ixv >> up : 0;
            xr[p][i] = *reinterpret_cast<const u32x4 *>(x + (unsigned)((pix[i] + iy * Win + ix) * Cin + ci0 + c * 8));
            xok[p] |= (unsigned)ok << i;
        }
#pragma unroll
        for (int j = 0; j < WL; ++j) wr[p][j] = *reinterpret_cast<const u32x4 *>(wnext + (long)(32 * j) * K9);
        wnext += 64;
        ci0 += 64;
        if (ci0 == Cin) { ci0 = 0; ++tap; }
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
    // its registers to the other LDS buffer, one barrier. The wait ahead of that move leaves the PF - 1 younger slabs in flight, across the
    // barrier too. The steady loop is free of conditions: every load and every move in it happens, so the compiler's wait counts are exact.
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
__global__ void __launch_bounds__(256) conv3x3_fold_kernel(const float *__restrict__ ws, T *__restrict__ y, long n4, int N, long MN, const ConvCold cold) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    const long off = q * 4;
    f32x4 a = *reinterpret_cast<const f32x4 *>(ws + off);
    for (int s = 1; s < cold.nsplit; ++s) a += *reinterpret_cast<const f32x4 *>(ws + s * MN + off);
    epilogue4<T>(a, cold, y, off, (int)(off % N));
}

// Tile width and K split per GEMM shape (M = B Ho Wo, N = Cout, K-slabs = 9 Cin / 64), measured on MI355X (tools/time_conv3x3.py --sweep,
// profiles/conv3x3_sweep_v2.md; conv3x3_sweep.md is the table of the one-slab loop): the SD1.5 UNet's convolutions at 2 and 16 rows. The fastest split keeps ~15 K-slabs per workgroup and
// 2 - 4 workgroups per CU; shapes not listed take the rule below (about 480 workgroups, at least 8 K-slabs per split).
struct ConvTune { int M, N, nslab, bn, nsplit; };
constexpr ConvTune CONV_TUNED[] = {
    // 2 rows (batch 1 with classifier-free guidance)
    // (the 160-wide cells: profiles/conv_wide160.md -- every shape where 160 beat the best 64 / 128 cell by more than the tool's 2 %)
    {8192, 320, 45, 160, 2}, {8192, 320, 90, 160, 2}, {8192, 320, 135, 160, 4}, {8192, 640, 90, 160, 1},
    {2048, 320, 45, 64, 6}, {2048, 640, 45, 64, 3}, {2048, 640, 90, 160, 4}, {2048, 640, 135, 160, 4}, {2048, 640, 180, 160, 4},
    {2048, 640, 270, 128, 6}, {2048, 1280, 180, 160, 4},
    {512, 640, 90, 64, 6}, {512, 1280, 90, 128, 6}, {512, 1280, 180, 160, 8}, {512, 1280, 270, 160, 8}, {512, 1280, 360, 160, 8},
    {128, 1280, 180, 64, 12}, {128, 1280, 360, 64, 24},
    // 16 rows (batch 8)
    {65536, 640, 90, 128, 1}, {16384, 1280, 180, 128, 1},
    {4096, 640, 90, 128, 3}, {4096, 1280, 90, 128, 3}, {4096, 1280, 180, 128, 3}, {4096, 1280, 270, 128, 3}, {4096, 1280, 360, 128, 3},
    {1024, 1280, 180, 128, 6}, {1024, 1280, 360, 128, 6},
};

struct ConvPlan {
    int M, Ho, Wo, bn, nsplit, nslab, ntiles;
};

bool plan_conv(const pww_conv_desc_t *d, ConvPlan *p) {
    if (!d || d->size < sizeof(pww_conv_desc_t)) { set_error("conv3x3: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return false; }
    const int up = d->upsample, s = d->stride;
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->B < 1 || d->Hin < 1 || d->Win < 1 || d->Cin < 64 || d->Cin % 64 != 0
        || d->Cout < 64 || (d->Cout % 64 != 0 && d->Cout % 160 != 0) || (s != 1 && s != 2) || (up != 0 && up != 1) || (up && s != 1) || d->Cin > 65536
        || d->Cout > 65536) {
        set_error("conv3x3: unsupported (dtype %d B %d %dx%d Cin %d Cout %d stride %d upsample %d): Cin a multiple of 64, Cout of 64 or 160, stride 1 or 2, "
                  "upsample only at stride 1", d->dtype, d->B, d->Hin, d->Win, d->Cin, d->Cout, s, up);
        return false;
    }
    const int Hv = d->Hin << up, Wv = d->Win << up;
#ifdef PWW_CONV_DOWN_UNIT
    if (s != 2 || up || Hv < 2 || Wv < 2) { set_error("conv3x3 (downsampler): stride 2, no upsample, H and W >= 2 (got stride %d, %dx%d)", s, d->Hin, d->Win); return false; }
    p->Ho = (Hv - 2) / 2 + 1;
    p->Wo = (Wv - 2) / 2 + 1;
#else
    p->Ho = (Hv - 1) / s + 1;
    p->Wo = (Wv - 1) / s + 1;
#endif
    const long M = (long)d->B * p->Ho * p->Wo;
    if ((long)d->B * d->Hin * d->Win * d->Cin >= (1L << 31) || M * d->Cout >= (1L << 31)) { set_error("conv3x3: tensor of 2^31 elements or more"); return false; }
    p->M = (int)M;
    p->nslab = 9 * d->Cin / 64;
    const ConvTune *tuned = nullptr;
#ifndef PWW_CONV_DOWN_UNIT      // (the table was measured on the padding-1 geometry, and some of its cells are the 160-wide tile)
    for (const ConvTune &t : CONV_TUNED)
        if (t.M == p->M && t.N == d->Cout && t.nslab == p->nslab) tuned = &t;
#endif
    p->bn = d->tile_n ? d->tile_n : tuned ? tuned->bn : (d->Cout % 128 == 0 ? 128 : d->Cout % 64 == 0 ? 64 : 160);
    if ((p->bn != 64 && p->bn != 128 && p->bn != 160) || d->Cout % p->bn != 0) { set_error("conv3x3: tile_n %d does not divide Cout %d", d->tile_n, d->Cout); return false; }
    p->ntiles = (p->M + CV_BM - 1) / CV_BM * (d->Cout / p->bn);
    int ns = d->splitk;
    if (ns <= 0 && tuned && p->bn == tuned->bn) ns = tuned->nsplit;
    if (ns <= 0) {          // about 480 workgroups (2 per CU), at least 8 K-slabs per split
        ns = (480 + p->ntiles / 2) / p->ntiles;
        if (ns > p->nslab / 8) ns = p->nslab / 8;
        if (ns < 1) ns = 1;
    }
    if (ns > p->nslab || ns > 64) { set_error("conv3x3: split %d exceeds the %d K-slabs (or 64)", ns, p->nslab); return false; }
    p->nsplit = ns;
    return true;
}

template <typename T>
int conv_launch(const ConvPlan &p, const pww_conv_desc_t *d, const void *x, const void *w, const void *bias, const void *residual, void *y, void *ws,
                hipStream_t stream) {
    const int N = d->Cout, HWo = p.Ho * p.Wo;
    ConvCold cold{bias, residual, p.nsplit, p.nslab | ((d->stride | (d->upsample << 4)) << 24),
                  p.nsplit > 1 ? partial_stores_through((size_t)p.nsplit * p.M * N * sizeof(float)) : 0};
    const T *xt = static_cast<const T *>(x), *wt = static_cast<const T *>(w);
    const dim3 grid(p.ntiles * p.nsplit), block(CV_THREADS);
    void *out = p.nsplit == 1 ? y : ws;
#ifdef PWW_CONV_WIDE_UNIT
    if (p.bn != 160) { set_error("conv3x3: tile_n %d is launched by libpww_hip.so (pww_conv3x3_fwd)", p.bn); return PWW_ENOTSUP; }
    constexpr size_t lds = 2 * (CV_BM + 160) * 128;
    static thread_local LdsRaised raised;       // (of conv3x3_kernel<T, 160>: this function is instantiated per T)
    if (raise_lds_limit(conv3x3_kernel<T, 160>, lds, raised)) return PWW_EHIP;
    launch_timed(conv3x3_kernel<T, 160>, grid, block, lds, stream, xt, wt, out, p.M, N, d->Cin, d->Hin, d->Win, p.Wo, HWo, cold);
#else
    if (p.bn == 160) { set_error("conv3x3: the 160-wide tile is launched by libpww_hip_convwide.so (pww_convwide_fwd)"); return PWW_ENOTSUP; }
    if (p.bn == 128) launch_timed(conv3x3_kernel<T, 128>, grid, block, 0, stream, xt, wt, out, p.M, N, d->Cin, d->Hin, d->Win, p.Wo, HWo, cold);
    else launch_timed(conv3x3_kernel<T, 64>, grid, block, 0, stream, xt, wt, out, p.M, N, d->Cin, d->Hin, d->Win, p.Wo, HWo, cold);
#endif
    if (p.nsplit == 1) return check_hip(hipGetLastError(), "conv3x3 launch");
    const long MN = (long)p.M * N, n4 = MN / 4;
    launch_timed(conv3x3_fold_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, static_cast<const float *>(ws), static_cast<T *>(y), n4,
                 N, MN, cold);
    return check_hip(hipGetLastError(), "conv3x3 fold launch");
}

bool al16(const void *a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace

// 1 when the plan of this descriptor (its tile_n, the table, or a Cout only 160 divides) is the 160-wide tile: the caller's choice of library
int conv3x3_plans_wide(const pww_conv_desc_t *d) {
    ConvPlan p;
    return plan_conv(d, &p) && p.bn == 160 ? 1 : 0;
}

size_t conv3x3_workspace_bytes(const pww_conv_desc_t *d) {
    ConvPlan p;
    if (!plan_conv(d, &p)) return 0;
    return p.nsplit > 1 ? (size_t)p.nsplit * p.M * d->Cout * sizeof(float) : 0;
}

int conv3x3_fwd(const void *x, const void *w, const void *bias, const void *residual, void *y, const pww_conv_desc_t *d, void *workspace,
                size_t workspace_bytes, hipStream_t stream) {
    ConvPlan p;
    if (!plan_conv(d, &p)) return PWW_ENOTSUP;
    // a descriptor is launched by exactly one of the two libraries this file is compiled into, decided by its plan alone
#ifdef PWW_CONV_WIDE_UNIT
    if (p.bn != 160) { set_error("conv3x3: tile_n %d is launched by libpww_hip.so (pww_conv3x3_fwd)", p.bn); return PWW_ENOTSUP; }
#else
    if (p.bn == 160) { set_error("conv3x3: the 160-wide tile is launched by libpww_hip_convwide.so (pww_convwide_fwd)"); return PWW_ENOTSUP; }
#endif
    if (!x || !w || !y) { set_error("conv3x3: x, w and y are required"); return PWW_EINVAL; }
    if (!al16(x) || !al16(w) || !al16(y) || (reinterpret_cast<uintptr_t>(bias) & 7) || (reinterpret_cast<uintptr_t>(residual) & 7)) {
        set_error("conv3x3: x, w, y must be 16-byte aligned, bias and residual 8-byte aligned");
        return PWW_EINVAL;
    }
    if (p.nsplit > 1 && (!workspace || !al16(workspace) || workspace_bytes < (size_t)p.nsplit * p.M * d->Cout * sizeof(float))) {
        set_error("conv3x3: split %d needs a 16-byte aligned workspace of %zu bytes (got %zu)", p.nsplit, (size_t)p.nsplit * p.M * d->Cout * sizeof(float),
                  workspace_bytes);
        return PWW_EINVAL;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    if (d->dtype == PWW_DTYPE_F16) return conv_launch<f16>(p, d, x, w, bias, residual, y, workspace, stream);
    return conv_launch<bf16>(p, d, x, w, bias, residual, y, workspace, stream);
}

}  // namespace pww
