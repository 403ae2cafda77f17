// The three pieces of the AutoencoderKL encoder that have no other kernel here (include/pww_hip_vaeenc.h):
//
// 1. pww_vaeenc_head_fwd: image -> conv_in (3 -> 128 channels, padding 1), channels_last out. An implicit GEMM whose whole contraction
//    (27 = 3 x 3 taps x 3 channels, k = 3 tap + channel) fits ONE mfma_f32_16x16x32 step, padded with zeros to 32. A wave owns 16
//    consecutive pixels per step: lane (fr, fq) gathers the 8 values k = 8 fq .. 8 fq + 7 of pixel fr (from the [B][3][H][W] tensor, or from
//    the uint8 image through the 256-entry table of normalised values; a tap outside the image is the VALUE 0) as the B operand; the weight
//    is the A operand, held in registers for the whole launch (8 tiles of 16 channels, 32 VGPRs). The rows of the tiles are dealt out so that
//    a lane's accumulators of tiles 2 p and 2 p + 1 are the 8 consecutive channels 32 p + 8 fq .. + 7 of its pixel: four 16-byte stores per
//    lane and step, 64 contiguous bytes per pixel and instruction. One rounding: T(acc + bias). The 8 MFMAs per 16 pixels are noise beside
//    the 256 bytes written per pixel; measured, the launch reaches 1.5 TB/s of stores at 512 x 512 (profiles/vae_encode.md), a quarter of the
//    write bound: the gather (8 element-sized loads per lane and step) and the 64-byte store segments are what is left to improve.
//
// 2. pww_vaeenc_down_*: the downsamplers. pww_conv.hip compiled with PWW_CONV_DOWN_UNIT: the product's implicit GEMM with the pad origin at
//    0 and Ho = (H - 2) / 2 + 1 (64- and 128-wide tiles, split-K with the fold launch). Not a second kernel: the same source.
//
// 3. pww_vaeenc_tail_*: conv_norm_out -> SiLU -> conv_out (512 -> 8) -> quant_conv (8 x 8) -> mean / logvar -> z, two launches.
//      statistics    grid (chunks <= 64, images): fp32 sum and sum of squares per group over the chunk's pixels, 4 pixel lanes per 8-channel
//                    slot folded through LDS in a fixed order; also the fp32 [channel][tap][8] copy of conv_out's weight, spread over the grid.
//      fused         a 512-thread workgroup owns 8 x 8 output pixels (lane = pixel); its eight waves split the 512 channels. A wave walks its
//                    64 channels in four GroupNorm groups of 16: it normalises the 10 x 10 halo of the group (fp32, SiLU; 0 outside the
//                    image -- the padding is that of the ACTIVATION) into its own LDS image [channel][pixel], then every lane reads its
//                    pixel's 9 neighbours per channel and multiplies each into 8 accumulators, the weights coming from scalar registers.
//                    The eight partial sums are added in wave order through LDS; wave 0 applies the bias, the 8 x 8 matrix, the clamp and
//                    the noise. Latency-bound (4096 pixels at 512 x 512): what it buys is two launches instead of about ten.
//
// Built as a library of its own (libpww_hip_vaeenc.so): host plumbing from pww_side_host.h, only pww_vaeenc_* visible.
#define PWW_SIDE_LIB "libpww_hip_vaeenc"
#include "pww_side_host.h"
#include "../../include/pww_hip_vaeenc.h"

#include <math.h>

#define PWW_VAEENC_API extern "C" __attribute__((visibility("default")))

#define PWW_CONV_DOWN_UNIT 1
#include "pww_conv.hip"

namespace pww {

namespace {

// ---- head --------------------------------------------------------------------------------------------------------------------------------
constexpr int VH_THREADS = 256, VH_C = PWW_VAEENC_HEAD_CHANNELS, VH_MAX_BLOCKS = 2048;

struct HeadArgs {
    const void *img, *table, *w, *bias;
    void *y;
    int H, W, M, form, ngroups;     // M = B H W pixels, in groups of 16
};

template <typename T>
__global__ void __launch_bounds__(VH_THREADS) vaeenc_head_kernel(const HeadArgs p) {
    typedef typename Vec<T>::v8 V8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int H = p.H, W = p.W, HW = H * W, M = p.M;
    // this lane's 8 contraction slots k = 8 fq + j = 3 tap + channel (k >= 27: the zero padding of the contraction)
    int dy[8], dx[8], ch[8];
    bool live[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * fq + j, tap = k / 3;
        live[j] = k < 27;
        ch[j] = k - 3 * tap;
        dy[j] = tap / 3 - 1;
        dx[j] = tap % 3 - 1;
    }
    // the weight as the A operand: row i of tile t is channel 32 (t >> 1) + 8 (i >> 2) + 4 (t & 1) + (i & 3), so that the lane that holds
    // rows 4 fq .. 4 fq + 3 of tiles 2 p and 2 p + 1 holds channels 32 p + 8 fq .. + 7
    V8 wf[8];
    {
        const T *w = reinterpret_cast<const T *>(p.w);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int co = 32 * (t >> 1) + 8 * (fr >> 2) + 4 * (t & 1) + (fr & 3);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int tap = (8 * fq + j) / 3;
                const T v = w[live[j] ? (co * 3 + ch[j]) * 9 + tap : 0];       // w[co][channel][ky][kx]
                wf[t][j] = live[j] ? v : (T)0.f;
            }
        }
    }
    float bf[4][8];
    {
        const T *bias = reinterpret_cast<const T *>(p.bias);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const V8 b = *reinterpret_cast<const V8 *>(bias + 32 * q + 8 * fq);
#pragma unroll
            for (int e = 0; e < 8; ++e) bf[q][e] = (float)b[e];
        }
    }
    const T *img = reinterpret_cast<const T *>(p.img), *table = reinterpret_cast<const T *>(p.table);
    const uint8_t *img8 = reinterpret_cast<const uint8_t *>(p.img);
    T *y = reinterpret_cast<T *>(p.y);
    for (int g = blockIdx.x * 4 + wave; g < p.ngroups; g += gridDim.x * 4) {
        const int m = g * 16 + fr, mc = min(m, M - 1);      // (a pixel past the end: clamped to load, not stored)
        const int b = mc / HW, rem = mc - b * HW, py = rem / W, px = rem - py * W;
        V8 xf;
        if (p.form == PWW_VAEENC_IN_UINT8) {                // (uniform)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int iy = py + dy[j], ix = px + dx[j];
                const bool ok = live[j] && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                const T v = table[img8[ok ? ((b * H + iy) * W + ix) * 3 + ch[j] : 0]];
                xf[j] = ok ? v : (T)0.f;                    // the padding is the VALUE 0, not pixel 0
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int iy = py + dy[j], ix = px + dx[j];
                const bool ok = live[j] && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                const T v = img[ok ? ((b * 3 + ch[j]) * H + iy) * W + ix : 0];
                xf[j] = ok ? v : (T)0.f;
            }
        }
        f32x4 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = mfma16(wf[t], xf, f32x4{0.f, 0.f, 0.f, 0.f});
        if (m < M) {
            T *yp = y + (long)m * VH_C + 8 * fq;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                V8 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = (T)(acc[2 * q][e] + bf[q][e]);
                    o[4 + e] = (T)(acc[2 * q + 1][e] + bf[q][4 + e]);
                }
                *reinterpret_cast<V8 *>(yp + 32 * q) = o;
            }
        }
    }
}

int head_check(const void *image, const void *table, const void *w, const void *bias, void *y, const pww_vaeenc_head_desc_t *d) {
    if (!d || d->size < sizeof(pww_vaeenc_head_desc_t)) { set_error("vaeenc_head: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    if (!image || !w || !bias || !y) { set_error("vaeenc_head: image, w, bias and y are required"); return PWW_EINVAL; }
    if (d->B < 1 || d->H < 1 || d->W < 1) { set_error("vaeenc_head: bad argument (B %d H %d W %d): sizes >= 1", d->B, d->H, d->W); return PWW_EINVAL; }
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || (d->in != PWW_VAEENC_IN_SAMPLE && d->in != PWW_VAEENC_IN_UINT8)) {
        set_error("vaeenc_head: unsupported (dtype %d in %d): F16 / BF16, the sample or the uint8 form", d->dtype, d->in);
        return PWW_ENOTSUP;
    }
    if (d->in == PWW_VAEENC_IN_UINT8 && !table) { set_error("vaeenc_head: the uint8 form needs the 256-entry table"); return PWW_EINVAL; }
    if ((int64_t)d->B * d->H * d->W * VH_C >= ((int64_t)1 << 31)) { set_error("vaeenc_head: output of 2^31 elements or more"); return PWW_ENOTSUP; }
    if (!aligned16(w) || !aligned16(bias) || !aligned16(y) || (d->in == PWW_VAEENC_IN_SAMPLE && !aligned16(image))) {
        set_error("vaeenc_head: image (sample form), w, bias and y must be 16-byte aligned");
        return PWW_ENOTSUP;
    }
    return PWW_OK;
}

// ---- tail --------------------------------------------------------------------------------------------------------------------------------
constexpr int VE_C = PWW_VAEENC_TAIL_CHANNELS, VE_G = PWW_VAEENC_TAIL_GROUPS, VE_THREADS = 512, VE_WAVES = 8, VE_STAT_THREADS = 256;
constexpr int VE_TILE = 8, VE_HALO = VE_TILE + 2, VE_PX = VE_HALO * VE_HALO;     // 8 x 8 output pixels, 10 x 10 inputs
constexpr int VE_PXS = 104;                 // LDS image: [channel][100 pixels + 4]
constexpr int VE_SUB = VE_C / VE_G;         // 16 channels: one GroupNorm group per pass
constexpr int VE_WROW = 72;                 // fp32 weight image: [channel][tap 9][output 8]

struct EncStatsArgs {
    const void *x, *w;
    float *part, *wf;
    int HW, ppc, nchunk;                    // pixels per image, per chunk; chunks per image
};

template <typename T>
__global__ void __launch_bounds__(VE_STAT_THREADS) vaeenc_tail_stats_kernel(const EncStatsArgs p) {
    typedef typename Vec<T>::v8 V8;
    __shared__ float red[4][64][2];
    const int chunk = blockIdx.x, b = blockIdx.y, t = threadIdx.x, c8 = t & 63, pl = t >> 6;
    const int pbeg = chunk * p.ppc, pend = min(pbeg + p.ppc, p.HW);
    const T *xb = reinterpret_cast<const T *>(p.x) + (long)b * p.HW * VE_C + c8 * 8;
    float s = 0.f, q = 0.f;
    for (int pix = pbeg + pl; pix < pend; pix += 4) {
        const V8 v = *reinterpret_cast<const V8 *>(xb + (long)pix * VE_C);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float f = (float)v[i];
            s += f;
            q += f * f;
        }
    }
    red[pl][c8][0] = s;
    red[pl][c8][1] = q;
    __syncthreads();
    if (t < 64) {       // t = 2 group + (0: sum, 1: sum of squares); a group is two 8-channel slots
        const int g = t >> 1, k = t & 1;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a += red[i][2 * g][k];
            a += red[i][2 * g + 1][k];
        }
        p.part[((long)b * p.nchunk + chunk) * 64 + t] = a;
    }
    if (p.w) {          // the weight the second launch reads: fp32 [channel][(ky 3 + kx)][o], every workgroup a slice of it
        const T *w = reinterpret_cast<const T *>(p.w);
        const int id = b * gridDim.x + chunk, nb = gridDim.x * gridDim.y;
        for (int i = id * VE_STAT_THREADS + t; i < VE_C * VE_WROW; i += nb * VE_STAT_THREADS) {
            const int c = i / VE_WROW, k = i - c * VE_WROW, tap = k >> 3, o = k & 7;
            p.wf[i] = (float)w[(o * VE_C + c) * 9 + tap];
        }
    }
}

struct EncTailArgs {
    const void *x, *gamma, *beta, *bias, *qw, *qb, *noise;
    const float *part, *wf;
    float *moments, *z;
    int H, W, nchunk;
    float eps, scale;
};

typedef const __attribute__((address_space(4))) float cfloat;     // constant address space: uniform reads become scalar loads

template <typename T>
__global__ void __launch_bounds__(VE_THREADS) vaeenc_tail_kernel(const EncTailArgs p) {
    typedef typename Vec<T>::v8 V8;
    __shared__ float gstat[2 * VE_G];
    __shared__ __attribute__((aligned(16))) float ab[2][VE_C];
    __shared__ __attribute__((aligned(16))) float act[VE_WAVES][VE_SUB * VE_PXS];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int b = blockIdx.z, H = p.H, W = p.W;
    if (t < VE_G) {     // the chunks of this image in their order; the moments in double
        const float *pp = p.part + (long)b * p.nchunk * 64 + 2 * t;
        double s = 0.0, q = 0.0;
        for (int ch = 0; ch < p.nchunk; ++ch) {
            s += (double)pp[ch * 64];
            q += (double)pp[ch * 64 + 1];
        }
        const double n = (double)H * W * VE_SUB, mean = s / n;
        double var = q / n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        gstat[2 * t] = (float)mean;
        gstat[2 * t + 1] = (float)(1.0 / sqrt(var + (double)p.eps));
    }
    __syncthreads();
    {                   // a = x A + B per channel (512 threads, 512 channels)
        const int g = t >> 4;
        const float A = gstat[2 * g + 1] * (float)reinterpret_cast<const T *>(p.gamma)[t];
        ab[0][t] = A;
        ab[1][t] = (float)reinterpret_cast<const T *>(p.beta)[t] - gstat[2 * g] * A;
    }
    __syncthreads();
    const int x0 = blockIdx.x * VE_TILE, y0 = blockIdx.y * VE_TILE, ty = lane >> 3, tx = lane & 7;
    const T *xb = reinterpret_cast<const T *>(p.x) + (long)b * H * W * VE_C;
    float *my = act[wave];
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = 0.f;
    for (int sub = 0; sub < 4; ++sub) {
        const int c0 = 64 * wave + VE_SUB * sub;
        // the group's halo, normalised: 100 pixels x 2 halves of 8 channels over the 64 lanes
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int it = lane + 64 * k;
            if (it < 2 * VE_PX) {
                const int hp = it >> 1, half = it & 1, hy = hp / VE_HALO, hx = hp - hy * VE_HALO;
                const int iy = y0 - 1 + hy, ix = x0 - 1 + hx, cb = c0 + 8 * half;
                const bool in = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                float a[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) a[i] = 0.f;         // outside the image: the padding is 0, not SiLU(norm(0))
                if (in) {
                    const V8 v = *reinterpret_cast<const V8 *>(xb + ((long)iy * W + ix) * VE_C + cb);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float f = (float)v[i] * ab[0][cb + i] + ab[1][cb + i];
                        a[i] = f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504f * f));
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) my[(8 * half + i) * VE_PXS + hp] = a[i];
            }
        }
        __syncthreads();
        cfloat *wc = (cfloat *)(p.wf) + c0 * VE_WROW;
        const float *ap = my + ty * VE_HALO + tx;
#pragma unroll 1        // (72 weights per channel in scalar registers: two channels' worth spill)
        for (int c = 0; c < VE_SUB; ++c) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float a = ap[c * VE_PXS + (tap / 3) * VE_HALO + tap % 3];
#pragma unroll
                for (int o = 0; o < 8; ++o) acc[o] += a * wc[c * VE_WROW + tap * 8 + o];
            }
        }
        __syncthreads();        // the image is rewritten by the next pass
    }
    // the eight partial sums in wave order (each wave's own slot: the start of its image)
#pragma unroll
    for (int o = 0; o < 8; ++o) my[o * 64 + lane] = acc[o];
    __syncthreads();
    const int oy = y0 + ty, ox = x0 + tx;
    if (wave == 0 && oy < H && ox < W) {
        const T *bias = reinterpret_cast<const T *>(p.bias), *qw = reinterpret_cast<const T *>(p.qw), *qb = reinterpret_cast<const T *>(p.qb);
        float m[8], q[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            float s = act[0][o * 64 + lane];
#pragma unroll
            for (int w = 1; w < VE_WAVES; ++w) s += act[w][o * 64 + lane];
            m[o] = s + (float)bias[o];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float s = (float)qb[i];
#pragma unroll
            for (int o = 0; o < 8; ++o) s += (float)qw[i * 8 + o] * m[o];
            q[i] = s;
        }
        const long HW = (long)H * W, pix = (long)oy * W + ox;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float mean = q[i], lv = fminf(fmaxf(q[4 + i], -30.f), 20.f);
            if (p.moments) {
                p.moments[((long)b * 8 + i) * HW + pix] = mean;
                p.moments[((long)b * 8 + 4 + i) * HW + pix] = lv;
            }
            float zz = mean;
            if (p.noise) zz += expf(0.5f * lv) * (float)reinterpret_cast<const T *>(p.noise)[((long)b * 4 + i) * HW + pix];
            p.z[((long)b * 4 + i) * HW + pix] = p.scale * zz;
        }
    }
}

struct EncTailPlan { int nchunk, ppc; size_t part_bytes, ws_bytes; };

// PWW_OK, or the code with the error text set. Nothing here touches the HIP runtime.
int enc_tail_plan(const pww_vaeenc_tail_desc_t *d, EncTailPlan *p) {
    if (!d || d->size < sizeof(pww_vaeenc_tail_desc_t)) { set_error("vaeenc_tail: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    if (d->B < 1 || d->H < 1 || d->W < 1) { set_error("vaeenc_tail: bad argument (B %d H %d W %d): sizes >= 1", d->B, d->H, d->W); return PWW_EINVAL; }
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->C != VE_C || !(d->eps > 0.f)) {
        set_error("vaeenc_tail: unsupported (dtype %d C %d eps %g): F16 / BF16, 512 channels, eps > 0", d->dtype, d->C, (double)d->eps);
        return PWW_ENOTSUP;
    }
    if ((int64_t)d->B * d->H * d->W * VE_C >= ((int64_t)1 << 31)) { set_error("vaeenc_tail: tensor of 2^31 elements or more"); return PWW_ENOTSUP; }
    if (d->B > 65535 || (d->H + VE_TILE - 1) / VE_TILE > 65535) { set_error("vaeenc_tail: more than 65535 images or row tiles"); return PWW_ENOTSUP; }
    const int HW = d->H * d->W;
    int nchunk = (HW + 63) / 64;
    nchunk = nchunk > PWW_VAEENC_TAIL_MAX_CHUNKS ? PWW_VAEENC_TAIL_MAX_CHUNKS : nchunk;
    p->ppc = (HW + nchunk - 1) / nchunk;
    p->nchunk = (HW + p->ppc - 1) / p->ppc;        // (no empty chunk)
    p->part_bytes = (size_t)d->B * p->nchunk * 64 * sizeof(float);
    p->ws_bytes = p->part_bytes + (size_t)VE_C * VE_WROW * sizeof(float);
    return PWW_OK;
}

int enc_tail_stats(const void *x, const void *w, const pww_vaeenc_tail_desc_t *d, void *ws, size_t ws_bytes, hipStream_t stream, EncTailPlan *plan) {
    const int rc = enc_tail_plan(d, plan);
    if (rc != PWW_OK) return rc;
    if (!x || !ws) { set_error("vaeenc_tail: x and the workspace are required"); return PWW_EINVAL; }
    if (ws_bytes < plan->ws_bytes) { set_error("vaeenc_tail: the workspace has %zu bytes, %zu are needed", ws_bytes, plan->ws_bytes); return PWW_EINVAL; }
    if (!aligned16(x) || !aligned16(ws)) { set_error("vaeenc_tail: x and the workspace must be 16-byte aligned"); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;
    float *part = static_cast<float *>(ws);
    const EncStatsArgs args{x, w, part, reinterpret_cast<float *>(static_cast<char *>(ws) + plan->part_bytes), d->H * d->W, plan->ppc, plan->nchunk};
    const dim3 grid(plan->nchunk, d->B), block(VE_STAT_THREADS);
    if (d->dtype == PWW_DTYPE_F16) launch_timed(vaeenc_tail_stats_kernel<f16>, grid, block, 0, stream, args);
    else launch_timed(vaeenc_tail_stats_kernel<bf16>, grid, block, 0, stream, args);
    return check_hip(hipGetLastError(), "vaeenc_tail statistics launch");
}

}  // namespace

int vaeenc_head_fwd(const void *image, const void *table, const void *w, const void *bias, void *y, const pww_vaeenc_head_desc_t *d, hipStream_t stream) {
    const int rc = head_check(image, table, w, bias, y, d);
    if (rc != PWW_OK) return rc;
    if (!arch_ok()) return PWW_ENOTSUP;
    const int M = d->B * d->H * d->W, ngroups = (M + 15) / 16;
    const HeadArgs args{image, table, w, bias, y, d->H, d->W, M, d->in, ngroups};
    const int blocks = (ngroups + 3) / 4;
    const dim3 grid(blocks < VH_MAX_BLOCKS ? blocks : VH_MAX_BLOCKS), block(VH_THREADS);
    if (d->dtype == PWW_DTYPE_F16) launch_timed(vaeenc_head_kernel<f16>, grid, block, 0, stream, args);
    else launch_timed(vaeenc_head_kernel<bf16>, grid, block, 0, stream, args);
    return check_hip(hipGetLastError(), "vaeenc_head launch");
}

// the downsampler's descriptor as the convolution's: stride 2, the geometry of this unit (PWW_CONV_DOWN_UNIT)
int down_desc(const pww_vaeenc_down_desc_t *d, pww_conv_desc_t *c) {
    if (!d || d->size < sizeof(pww_vaeenc_down_desc_t)) { set_error("vaeenc_down: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    if (d->B < 1 || d->H < 2 || d->W < 2 || d->Cin < 64 || d->Cin % 64 != 0 || d->Cout < 64 || d->Cout % 64 != 0
        || (d->tile_n != 0 && d->tile_n != 64 && d->tile_n != 128)) {
        set_error("vaeenc_down: unsupported (B %d %dx%d Cin %d Cout %d tile_n %d): B >= 1, H and W >= 2, Cin and Cout multiples of 64, tile_n 0, 64 or 128",
                  d->B, d->H, d->W, d->Cin, d->Cout, d->tile_n);
        return PWW_ENOTSUP;
    }
    *c = pww_conv_desc_t{(uint32_t)sizeof(pww_conv_desc_t), d->dtype, d->B, d->H, d->W, d->Cin, d->Cout, 2, 0, d->tile_n, d->splitk, 0};
    return PWW_OK;
}

int vaeenc_tail_fwd(const void *x, const void *gamma, const void *beta, const void *w, const void *bias, const void *qw, const void *qb, const void *noise,
                    void *moments, void *z, const pww_vaeenc_tail_desc_t *d, void *ws, size_t ws_bytes, hipStream_t stream) {
    if (d && d->size >= sizeof(pww_vaeenc_tail_desc_t) && (!gamma || !beta || !w || !bias || !qw || !qb || !z)) {
        set_error("vaeenc_tail: gamma, beta, w, bias, qw, qb and z are required");
        return PWW_EINVAL;
    }
    EncTailPlan plan;
    const int rc = enc_tail_stats(x, w, d, ws, ws_bytes, stream, &plan);
    if (rc != PWW_OK) return rc;
    const EncTailArgs args{x, gamma, beta, bias, qw, qb, noise, static_cast<const float *>(ws),
                           reinterpret_cast<const float *>(static_cast<const char *>(ws) + plan.part_bytes), static_cast<float *>(moments),
                           static_cast<float *>(z), d->H, d->W, plan.nchunk, d->eps, d->scale};
    const dim3 grid((d->W + VE_TILE - 1) / VE_TILE, (d->H + VE_TILE - 1) / VE_TILE, d->B), block(VE_THREADS);
    if (d->dtype == PWW_DTYPE_F16) launch_timed(vaeenc_tail_kernel<f16>, grid, block, 0, stream, args);
    else launch_timed(vaeenc_tail_kernel<bf16>, grid, block, 0, stream, args);
    return check_hip(hipGetLastError(), "vaeenc_tail launch");
}

}  // namespace pww

PWW_VAEENC_API int pww_vaeenc_version(void) { return PWW_VAEENC_VERSION; }
PWW_VAEENC_API const char *pww_vaeenc_last_error(void) { return pww::last_error(); }
PWW_VAEENC_API int pww_vaeenc_head_fwd(const void *image, const void *table, const void *w, const void *bias, void *y, const pww_vaeenc_head_desc_t *desc,
                                       void *stream) {
    return pww::vaeenc_head_fwd(image, table, w, bias, y, desc, static_cast<hipStream_t>(stream));
}
PWW_VAEENC_API size_t pww_vaeenc_down_workspace_bytes(const pww_vaeenc_down_desc_t *desc) {
    pww_conv_desc_t c;
    return pww::down_desc(desc, &c) == PWW_OK ? pww::conv3x3_workspace_bytes(&c) : 0;
}
PWW_VAEENC_API int pww_vaeenc_down_fwd(const void *x, const void *w, const void *bias, void *y, const pww_vaeenc_down_desc_t *desc, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    pww_conv_desc_t c;
    const int rc = pww::down_desc(desc, &c);
    if (rc != PWW_OK) return rc;
    return pww::conv3x3_fwd(x, w, bias, nullptr, y, &c, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
PWW_VAEENC_API size_t pww_vaeenc_tail_workspace_bytes(const pww_vaeenc_tail_desc_t *desc) {
    pww::EncTailPlan plan;
    return pww::enc_tail_plan(desc, &plan) == PWW_OK ? plan.ws_bytes : 0;
}
PWW_VAEENC_API int pww_vaeenc_tail_chunks(const pww_vaeenc_tail_desc_t *desc) {
    pww::EncTailPlan plan;
    return pww::enc_tail_plan(desc, &plan) == PWW_OK ? plan.nchunk : 0;
}
PWW_VAEENC_API int pww_vaeenc_tail_stats(const void *x, const void *w, const pww_vaeenc_tail_desc_t *desc, void *ws, size_t ws_bytes, void *stream) {
    pww::EncTailPlan plan;
    return pww::enc_tail_stats(x, w, desc, ws, ws_bytes, static_cast<hipStream_t>(stream), &plan);
}
PWW_VAEENC_API int pww_vaeenc_tail_fwd(const void *x, const void *gamma, const void *beta, const void *w, const void *bias, const void *qw, const void *qb,
                                       const void *noise, void *moments, void *z, const pww_vaeenc_tail_desc_t *desc, void *ws, size_t ws_bytes,
                                       void *stream) {
    return pww::vaeenc_tail_fwd(x, gamma, beta, w, bias, qw, qb, noise, moments, z, desc, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
