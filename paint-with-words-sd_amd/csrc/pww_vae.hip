// The two pieces of the AutoencoderKL decoder that have no other kernel here (include/pww_hip_vae.h):
//
// 1. pww_vae_attn_fwd: the mid block's attention -- ONE head of dim 512, N = H W tokens -- flash-style on MFMA.
//    A 32-row accumulator 512 wide is 256 fp32 registers per lane, so the structure of pww_attn.hip (d <= 160 in one wave's registers) does
//    not carry over. Here a 256-thread workgroup owns 32 queries, and its four waves split BOTH products by head-dim quarter:
//      S^T partial   wave w contracts over d in [128 w, 128 w + 128): 8 x mfma_32x32x16 with the K rows as the A operand and Q^T as B (in
//                    registers for the whole launch). The [32 keys][128] slice belongs to this wave alone; it is loaded 256 contiguous bytes
//                    per key and instruction and turned into operand layout through a region of LDS only this wave touches -- no barrier:
//                    LDS operations of one wave execute in order. (Loaded in operand layout straight from global memory, every instruction
//                    touched 64 cache lines for 16 bytes each: 2.3 x slower at N = 4096, profiles/vae_decode.md.) S^T, not S: each lane then
//                    holds 16 keys of ONE query, and the row maximum / sum are 16 registers and one exchange with lane ^ 32.
//      reduction     the four partials go through LDS once per key block ([wave][register quad][lane] float4: 16-byte accesses at the
//                    lane's own slot); every wave adds them in the same order and runs the same online softmax on the same numbers, so the
//                    four waves agree bit for bit on the maximum, the rescale and P.
//      O^T           wave w owns output columns [128 w, 128 w + 128): 4 tiles x 2 k-steps of mfma_32x32x16 with V^T (LDS) as A and P^T
//                    (registers, rounded to the storage type) as B. The keys a lane holds after the first product are
//                    16 s + 8 (j >> 2) + 4 h + (j & 3) for k-slot (s, h, j) (pww_common.h: swap23); the V image is staged in that order.
//      V staging     the product sums over V's ROW index, so the operand is a transpose: each thread loads 8 keys x 8 columns (8 coalesced
//                    16-byte loads: a wave reads whole 1 KB rows), transposes them in registers and stores 8 x 16 bytes into the
//                    [column][32 keys] image (80-byte rows + 16 bytes per 16 columns: the 16-byte reads of a 16-lane group and the stores
//                    both spread over the banks).
//    The two shared LDS regions are double-buffered (2 x 56.5 KB, + 4 x 8.5 KB of K slices), so a key block costs ONE barrier; the K and V
//    loads of the next block are issued right behind it (in front of it the barrier's fence would wait for them) and land behind the
//    softmax and the second product.
//
// 2. pww_vae_tail_*: conv_norm_out -> SiLU -> conv_out (128 -> 3) -> image, two launches.
//      statistics    grid (chunks <= 64, images): fp32 sum and sum of squares per group over the chunk's pixels, 16 pixel lanes per 8-channel
//                    slot folded through LDS in a fixed order; also the fp32 [channel][27] copy of the weight.
//      fused         a workgroup owns 8 output rows x 62 columns; its four waves split the 128 channels, lane = input column (64 with the
//                    halo). Walking down the 10 input rows each lane normalises its pixel's 32 channels once (fp32, SiLU), and multiplies
//                    them into 27 rolling accumulators (3 output rows x 3 horizontal taps x 3 outputs; weights from scalar registers): a
//                    pixel outside the image contributes 0 -- the padding is that of the ACTIVATION. A finished output row's 9 values per
//                    lane are added over the four waves, and over the neighbouring lanes for the horizontal taps, through LDS (double
//                    buffered: one barrier per row); bias, then the .sample form or the 8-bit image.
//
// Built as a library of its own (libpww_hip_vae.so): host plumbing from pww_side_host.h, only pww_vae_* visible.
#define PWW_SIDE_LIB "libpww_hip_vae"
#include "pww_side_host.h"
#include "../../include/pww_hip_vae.h"

#include <math.h>

#define PWW_VAE_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

// ---- attention ---------------------------------------------------------------------------------------------------------------------------
constexpr int VA_THREADS = 256, VA_BM = 32, VA_BN = 32, VA_D = PWW_VAE_HEAD_DIM;
constexpr int VA_SP_BYTES = 4 * 4 * 64 * 16;                    // partial scores: [wave][register quad][lane] float4
constexpr int VA_VT_ROW = 80;                                   // 32 keys of one column + 16 bytes
constexpr int VA_VT_BYTES = VA_D * VA_VT_ROW + (VA_D / 16) * 16;
constexpr int VA_STAGE = VA_SP_BYTES + VA_VT_BYTES;             // 57 856
constexpr int VA_KT_ROW = 272;                                  // 128 elements of one key + 16 bytes: 16-byte reads of 16 keys hit 16 slots
constexpr int VA_KT_BYTES = VA_BN * VA_KT_ROW;                  // 8 704 per wave
constexpr int VA_LDS = 2 * VA_STAGE + 4 * VA_KT_BYTES;          // 150 528 of the CU's 160 KB

struct VaeAttnArgs {
    const void *q, *k, *v;
    void *o;
    long qbs, qrs, kbs, krs, vbs, vrs, obs, ors;    // batch / row strides, in elements
    int N;
    float scale_log2;                               // scale * log2(e)
};

__device__ __forceinline__ int vt_offset(int col) { return col * VA_VT_ROW + (col >> 4) * 16; }

template <typename T>
__global__ void __launch_bounds__(VA_THREADS) vae_attn_kernel(const VaeAttnArgs p) {
    typedef typename Vec<T>::v8 V8;
    typedef typename Vec<T>::v4 V4;
    char *lds = launch_lds();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, q0 = blockIdx.x * VA_BM, N = p.N;
    const T *qb = reinterpret_cast<const T *>(p.q) + (long)b * p.qbs;
    const T *kb = reinterpret_cast<const T *>(p.k) + (long)b * p.kbs;
    const T *vb = reinterpret_cast<const T *>(p.v) + (long)b * p.vbs;
    // k-slot (s, h, j) of this wave's contraction is head-dim element 128 wave + 64 h + 8 s + j for Q and K alike: a lane reads 128
    // consecutive bytes of its row over the 8 steps. Rows past N are clamped (their scores are masked / their outputs not stored).
    const int dcol = 128 * wave + 64 * h;
    V8 qf[8];
    {
        const T *qp = qb + (long)min(q0 + l31, N - 1) * p.qrs + dcol;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const V8 *>(qp + 8 * s);
    }
    f32x16 oacc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int nblk = (N + VA_BN - 1) / VA_BN;

    V8 kf[8], vf[8];
    char *kt = lds + 2 * VA_STAGE + wave * VA_KT_BYTES;         // this wave's K slice: [32 keys][128 + 8] elements, its own and nobody else's
    auto load_kv = [&](int blk) {
        // 4 keys x 256 contiguous bytes per load (an operand-layout load would touch 64 lines of 16 bytes each)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = blk * VA_BN + 4 * i + (lane >> 4);
            kf[i] = *reinterpret_cast<const V8 *>(kb + (long)min(key, N - 1) * p.krs + 128 * wave + 8 * (lane & 15));
        }
        // this wave stages image positions 8 wave .. 8 wave + 7: keys 16 (wave >> 1) + 8 (jj >> 2) + 4 (wave & 1) + (jj & 3)
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int key = blk * VA_BN + 16 * (wave >> 1) + 8 * (jj >> 2) + 4 * (wave & 1) + (jj & 3);
            vf[jj] = *reinterpret_cast<const V8 *>(vb + (long)min(key, N - 1) * p.vrs + 8 * lane);
        }
    };
    load_kv(0);

    for (int blk = 0; blk < nblk; ++blk) {
        char *stage = lds + (blk & 1) * VA_STAGE;
        f32x4 *sp = reinterpret_cast<f32x4 *>(stage);
        char *vt = stage + VA_SP_BYTES;
        // this wave's part of S^T: D[key][query]
        // (the K slice through the wave's own LDS region: LDS operations of one wave execute in order, so no workgroup barrier is involved)
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<V8 *>(kt + (4 * i + (lane >> 4)) * VA_KT_ROW + 16 * (lane & 15)) = kf[i];
        __builtin_amdgcn_wave_barrier();
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int st = 0; st < 8; ++st) s = mfma32(*reinterpret_cast<const V8 *>(kt + l31 * VA_KT_ROW + 2 * (64 * h + 8 * st)), qf[st], s);
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) sp[(wave * 4 + rq) * 64 + lane] = f32x4{s[4 * rq], s[4 * rq + 1], s[4 * rq + 2], s[4 * rq + 3]};
        // V^T image: column 8 lane + c, positions 8 wave .. + 7
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            V8 t;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) t[jj] = vf[jj][c];
            *reinterpret_cast<V8 *>(vt + vt_offset(8 * lane + c) + 16 * wave) = t;
        }
        __syncthreads();
        // the next block's K and V: issued BEHIND the barrier (its fence would wait for them) and consumed after the second product
        if (blk + 1 < nblk) load_kv(blk + 1);

        // the whole S^T: the four parts in a fixed order, the same in every wave
        float sv[16];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            f32x4 a = sp[rq * 64 + lane];
            a += sp[(4 + rq) * 64 + lane];
            a += sp[(8 + rq) * 64 + lane];
            a += sp[(12 + rq) * 64 + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[4 * rq + i] = a[i];
        }
        const int kbase = blk * VA_BN + 4 * h;
        float mb = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kbase + (r & 3) + 8 * (r >> 2);
            sv[r] = key < N ? sv[r] * p.scale_log2 : -INFINITY;
            mb = fmaxf(mb, sv[r]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float m_new = fmaxf(m_run, mb);           // finite: every block has a live key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float psum = 0.f;
        V8 pf[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pr = __builtin_amdgcn_exp2f(sv[r] - m_new);
            psum += pr;
            pf[r >> 3][r & 7] = (T)pr;
        }
        l_run = l_run * alpha + psum;
        if (__any(m_new > m_run)) {                     // (wave-uniform) a lane's accumulators all belong to its query
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
        }
        m_run = m_new;
        // O^T[column][query] += V^T P^T
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const char *vp = vt + vt_offset(128 * wave + 32 * t + l31) + 16 * h;
#pragma unroll
            for (int st = 0; st < 2; ++st) oacc[t] = mfma32(*reinterpret_cast<const V8 *>(vp + 32 * st), pf[st], oacc[t]);
        }
    }

    const float l_all = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.f / l_all;
    const int qrow = q0 + l31;
    if (qrow < N) {
        T *op = reinterpret_cast<T *>(p.o) + (long)b * p.obs + (long)qrow * p.ors + 128 * wave + 4 * h;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                V4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (T)(oacc[t][4 * rq + i] * inv);
                *reinterpret_cast<V4 *>(op + 32 * t + 8 * rq) = o;
            }
    }
}

int attn_check(const void *q, const void *k, const void *v, void *o, const pww_vae_attn_desc_t *d) {
    if (!d || d->size < sizeof(pww_vae_attn_desc_t)) { set_error("vae_attn: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    if (!q || !k || !v || !o) { set_error("vae_attn: q, k, v and o are required"); return PWW_EINVAL; }
    if (d->B < 1 || d->N < 1) { set_error("vae_attn: bad argument (B %d N %d): sizes >= 1", d->B, d->N); return PWW_EINVAL; }
    if (d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) { set_error("vae_attn: unsupported dtype %d (F16 / BF16)", d->dtype); return PWW_ENOTSUP; }
    if (d->D != VA_D) { set_error("vae_attn: head dim %d is not %d", d->D, VA_D); return PWW_ENOTSUP; }
    const int64_t strides[8] = {d->q_batch_stride, d->q_row_stride, d->k_batch_stride, d->k_row_stride, d->v_batch_stride, d->v_row_stride,
                                d->o_batch_stride, d->o_row_stride};
    const int64_t lim = (int64_t)1 << 31;
    for (int i = 0; i < 8; ++i) {
        const bool row = i & 1;
        if ((strides[i] & 7) || strides[i] < 0 || (row && strides[i] < VA_D)) {
            set_error("vae_attn: stride %d (%ld) must be a multiple of 8 elements%s", i, (long)strides[i], row ? " and at least 512" : "");
            return PWW_ENOTSUP;
        }
        if (row && ((int64_t)(d->N - 1) * strides[i] + VA_D >= lim || (int64_t)(d->B - 1) * strides[i - 1] + (int64_t)(d->N - 1) * strides[i] + VA_D >= lim)) {
            set_error("vae_attn: extent of 2^31 elements or more");
            return PWW_ENOTSUP;
        }
    }
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o)) { set_error("vae_attn: q, k, v and o must be 16-byte aligned"); return PWW_ENOTSUP; }
    if (d->B > 65535) { set_error("vae_attn: more than 65535 images"); return PWW_ENOTSUP; }
    return PWW_OK;
}

template <typename T>
int attn_launch(const pww_vae_attn_desc_t *d, const VaeAttnArgs &args, hipStream_t stream) {
    static thread_local LdsRaised raised;
    if (raise_lds_limit(vae_attn_kernel<T>, VA_LDS, raised)) return PWW_EHIP;
    const dim3 grid((d->N + VA_BM - 1) / VA_BM, d->B), block(VA_THREADS);
    launch_timed(vae_attn_kernel<T>, grid, block, VA_LDS, stream, args);
    return check_hip(hipGetLastError(), "vae_attn launch");
}

// ---- tail --------------------------------------------------------------------------------------------------------------------------------
constexpr int VT_C = PWW_VAE_TAIL_CHANNELS, VT_G = PWW_VAE_TAIL_GROUPS, VT_THREADS = 256;
constexpr int VT_TH = 8, VT_TW = 62;        // output rows / columns of a workgroup (64 input columns with the halo)
constexpr int VT_WROW = 28;                 // fp32 weight image: [channel][27 + 1]

struct TailStatsArgs {
    const void *x, *w;
    float *part, *wf;
    int HW, ppc, nchunk;                    // pixels per image, per chunk; chunks per image
};

template <typename T>
__global__ void __launch_bounds__(VT_THREADS) vae_tail_stats_kernel(const TailStatsArgs p) {
    typedef typename Vec<T>::v8 V8;
    __shared__ float red[16][16][4];
    const int chunk = blockIdx.x, b = blockIdx.y, t = threadIdx.x, c8 = t & 15, pl = t >> 4;
    const int pbeg = chunk * p.ppc, pend = min(pbeg + p.ppc, p.HW);
    const T *xb = reinterpret_cast<const T *>(p.x) + (long)b * p.HW * VT_C + c8 * 8;
    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
    for (int pix = pbeg + pl; pix < pend; pix += 16) {
        const V8 v = *reinterpret_cast<const V8 *>(xb + (long)pix * VT_C);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float f = (float)v[i], g = (float)v[4 + i];
            s0 += f; q0 += f * f;
            s1 += g; q1 += g * g;
        }
    }
    red[pl][c8][0] = s0; red[pl][c8][1] = q0; red[pl][c8][2] = s1; red[pl][c8][3] = q1;
    __syncthreads();
    if (t < 64) {       // t = 2 group + (0: sum, 1: sum of squares)
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) a += red[i][t >> 2][t & 3];
        p.part[((long)b * p.nchunk + chunk) * 64 + t] = a;
    }
    if (p.w && chunk == 0 && b == 0) {      // the weight the second launch reads: fp32 [channel][(dy 3 + dx) 3 + o]
        const T *w = reinterpret_cast<const T *>(p.w);
        for (int i = t; i < VT_C * VT_WROW; i += VT_THREADS) {
            const int c = i / VT_WROW, k = i - c * VT_WROW;
            const int dy = k / 9, dx = (k / 3) % 3, o = k % 3;
            p.wf[i] = k < 27 ? (float)w[((o * VT_C + c) * 3 + dy) * 3 + dx] : 0.f;
        }
    }
}

struct TailArgs {
    const void *x, *gamma, *beta, *bias;
    const float *part, *wf;
    void *out;
    int H, W, nchunk, form;
    float eps;
};

typedef const __attribute__((address_space(4))) float cfloat;     // constant address space: uniform reads become scalar loads

template <typename T>
__global__ void __launch_bounds__(VT_THREADS) vae_tail_kernel(const TailArgs p) {
    typedef typename Vec<T>::v8 V8;
    __shared__ float gstat[2 * VT_G];
    __shared__ float red[2][4][9][64];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int b = blockIdx.z, H = p.H, W = p.W;
    if (t < VT_G) {     // the chunks of this image in their order; the moments in double
        const float *pp = p.part + (long)b * p.nchunk * 64 + 2 * t;
        double s = 0.0, q = 0.0;
        for (int ch = 0; ch < p.nchunk; ++ch) {
            s += (double)pp[ch * 64];
            q += (double)pp[ch * 64 + 1];
        }
        const double n = (double)H * W * (VT_C / VT_G), mean = s / n;
        double var = q / n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        gstat[2 * t] = (float)mean;
        gstat[2 * t + 1] = (float)(1.0 / sqrt(var + (double)p.eps));
    }
    __syncthreads();
    // this wave's 32 channels: a = x A + B
    float A[32], Bc[32];
    {
        const T *gamma = reinterpret_cast<const T *>(p.gamma) + 32 * wave, *beta = reinterpret_cast<const T *>(p.beta) + 32 * wave;
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            const int g = 8 * wave + (c >> 2);
            A[c] = gstat[2 * g + 1] * (float)gamma[c];
            Bc[c] = (float)beta[c] - gstat[2 * g] * A[c];
        }
    }
    cfloat *wc = (cfloat *)(p.wf) + 32 * wave * VT_WROW;
    const int x0 = blockIdx.x * VT_TW, y0 = blockIdx.y * VT_TH;
    const int xi = x0 - 1 + lane;
    const bool xin = xi >= 0 && xi < W;
    const int nrows = min(VT_TH, H - y0) + 2;
    const T *xb = reinterpret_cast<const T *>(p.x) + (long)b * H * W * VT_C + 32 * wave;
    const T *bias = reinterpret_cast<const T *>(p.bias);
    float U[3][9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) U[i][k] = 0.f;
    int ph = 0;
    for (int r = 0; r < nrows; ++r) {
        const int yi = y0 - 1 + r;
        if (yi >= 0 && yi < H) {        // (uniform) a row outside the image contributes nothing
            const T *xp = xb + ((long)yi * W + min(max(xi, 0), W - 1)) * VT_C;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const V8 v = *reinterpret_cast<const V8 *>(xp + 8 * cc);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int c = 8 * cc + i;
                    float a = (float)v[i] * A[c] + Bc[c];
                    a = a * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504f * a));
                    a = xin ? a : 0.f;      // a column outside the image: the padding is 0, not SiLU(norm(0))
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        U[0][k] += a * wc[c * VT_WROW + k];            // dy = 0: output row yi + 1
                        U[1][k] += a * wc[c * VT_WROW + 9 + k];        // dy = 1: output row yi
                        U[2][k] += a * wc[c * VT_WROW + 18 + k];       // dy = 2: output row yi - 1, complete with this
                    }
                }
            }
        }
        if (r >= 2) {                   // (uniform) output row yi - 1 is complete
#pragma unroll
            for (int k = 0; k < 9; ++k) red[ph][wave][k][lane] = U[2][k];
            __syncthreads();
            if (wave == (r & 3)) {
                const int yo = yi - 1, xo = xi;
                float o[3];
#pragma unroll
                for (int oo = 0; oo < 3; ++oo) o[oo] = 0.f;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int ln = min(max(lane + dx - 1, 0), 63);
#pragma unroll
                    for (int oo = 0; oo < 3; ++oo) {
                        float s = red[ph][0][dx * 3 + oo][ln];
                        s += red[ph][1][dx * 3 + oo][ln];
                        s += red[ph][2][dx * 3 + oo][ln];
                        s += red[ph][3][dx * 3 + oo][ln];
                        o[oo] += s;
                    }
                }
                if (lane >= 1 && lane <= VT_TW && xo < W) {
#pragma unroll
                    for (int oo = 0; oo < 3; ++oo) {
                        const float y = o[oo] + (float)bias[oo];
                        if (p.form == PWW_VAE_OUT_UINT8) {
                            const float u = rintf(255.f * fminf(fmaxf(y * 0.5f + 0.5f, 0.f), 1.f));
                            reinterpret_cast<uint8_t *>(p.out)[(((long)b * H + yo) * W + xo) * 3 + oo] = (uint8_t)u;
                        } else {
                            reinterpret_cast<T *>(p.out)[(((long)b * 3 + oo) * H + yo) * W + xo] = (T)y;
                        }
                    }
                }
            }
            ph ^= 1;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            U[2][k] = U[1][k];
            U[1][k] = U[0][k];
            U[0][k] = 0.f;
        }
    }
}

struct TailPlan { int nchunk, ppc; size_t part_bytes, ws_bytes; };

// PWW_OK, or the code with the error text set. Nothing here touches the HIP runtime.
int tail_plan(const pww_vae_tail_desc_t *d, TailPlan *p) {
    if (!d || d->size < sizeof(pww_vae_tail_desc_t)) { set_error("vae_tail: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    if (d->B < 1 || d->H < 1 || d->W < 1) { set_error("vae_tail: bad argument (B %d H %d W %d): sizes >= 1", d->B, d->H, d->W); return PWW_EINVAL; }
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->C != VT_C || (d->out != PWW_VAE_OUT_SAMPLE && d->out != PWW_VAE_OUT_UINT8)
        || !(d->eps > 0.f)) {
        set_error("vae_tail: unsupported (dtype %d C %d out %d eps %g): F16 / BF16, 128 channels, the sample or the uint8 form, eps > 0", d->dtype, d->C, d->out,
                  (double)d->eps);
        return PWW_ENOTSUP;
    }
    if ((int64_t)d->B * d->H * d->W * VT_C >= ((int64_t)1 << 31)) { set_error("vae_tail: tensor of 2^31 elements or more"); return PWW_ENOTSUP; }
    if (d->B > 65535 || (d->H + VT_TH - 1) / VT_TH > 65535) { set_error("vae_tail: more than 65535 images or row tiles"); return PWW_ENOTSUP; }
    const int HW = d->H * d->W;
    int nchunk = (HW + 255) / 256;
    nchunk = nchunk > PWW_VAE_TAIL_MAX_CHUNKS ? PWW_VAE_TAIL_MAX_CHUNKS : nchunk;
    p->ppc = (HW + nchunk - 1) / nchunk;
    p->nchunk = (HW + p->ppc - 1) / p->ppc;        // (no empty chunk)
    p->part_bytes = (size_t)d->B * p->nchunk * 64 * sizeof(float);
    p->ws_bytes = p->part_bytes + (size_t)VT_C * VT_WROW * sizeof(float);
    return PWW_OK;
}

int tail_stats(const void *x, const void *w, const pww_vae_tail_desc_t *d, void *ws, size_t ws_bytes, hipStream_t stream, TailPlan *plan) {
    const int rc = tail_plan(d, plan);
    if (rc != PWW_OK) return rc;
    if (!x || !ws) { set_error("vae_tail: x and the workspace are required"); return PWW_EINVAL; }
    if (ws_bytes < plan->ws_bytes) { set_error("vae_tail: the workspace has %zu bytes, %zu are needed", ws_bytes, plan->ws_bytes); return PWW_EINVAL; }
    if (!aligned16(x) || !aligned16(ws)) { set_error("vae_tail: x and the workspace must be 16-byte aligned"); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;
    float *part = static_cast<float *>(ws);
    const TailStatsArgs args{x, w, part, reinterpret_cast<float *>(static_cast<char *>(ws) + plan->part_bytes), d->H * d->W, plan->ppc, plan->nchunk};
    const dim3 grid(plan->nchunk, d->B), block(VT_THREADS);
    if (d->dtype == PWW_DTYPE_F16) launch_timed(vae_tail_stats_kernel<f16>, grid, block, 0, stream, args);
    else launch_timed(vae_tail_stats_kernel<bf16>, grid, block, 0, stream, args);
    return check_hip(hipGetLastError(), "vae_tail statistics launch");
}

}  // namespace

int vae_attn_fwd(const void *q, const void *k, const void *v, void *o, const pww_vae_attn_desc_t *d, hipStream_t stream) {
    const int rc = attn_check(q, k, v, o, d);
    if (rc != PWW_OK) return rc;
    if (!arch_ok()) return PWW_ENOTSUP;
    const float scale = d->scale > 0.f ? d->scale : 1.f / sqrtf((float)VA_D);
    const VaeAttnArgs args{q, k, v, o, d->q_batch_stride, d->q_row_stride, d->k_batch_stride, d->k_row_stride, d->v_batch_stride, d->v_row_stride,
                           d->o_batch_stride, d->o_row_stride, d->N, scale * 1.44269504088896341f};
    if (d->dtype == PWW_DTYPE_F16) return attn_launch<f16>(d, args, stream);
    return attn_launch<bf16>(d, args, stream);
}

int vae_tail_fwd(const void *x, const void *gamma, const void *beta, const void *w, const void *bias, void *out, const pww_vae_tail_desc_t *d,
                 void *ws, size_t ws_bytes, hipStream_t stream) {
    if (d && d->size >= sizeof(pww_vae_tail_desc_t) && (!gamma || !beta || !w || !bias || !out)) {
        set_error("vae_tail: gamma, beta, w, bias and out are required");
        return PWW_EINVAL;
    }
    TailPlan plan;
    const int rc = tail_stats(x, w, d, ws, ws_bytes, stream, &plan);
    if (rc != PWW_OK) return rc;
    const TailArgs args{x, gamma, beta, bias, static_cast<const float *>(ws),
                        reinterpret_cast<const float *>(static_cast<const char *>(ws) + plan.part_bytes), out, d->H, d->W, plan.nchunk, d->out, d->eps};
    const dim3 grid((d->W + VT_TW - 1) / VT_TW, (d->H + VT_TH - 1) / VT_TH, d->B), block(VT_THREADS);
    if (d->dtype == PWW_DTYPE_F16) launch_timed(vae_tail_kernel<f16>, grid, block, 0, stream, args);
    else launch_timed(vae_tail_kernel<bf16>, grid, block, 0, stream, args);
    return check_hip(hipGetLastError(), "vae_tail launch");
}

}  // namespace pww

PWW_VAE_API int pww_vae_version(void) { return PWW_VAE_VERSION; }
PWW_VAE_API const char *pww_vae_last_error(void) { return pww::last_error(); }
PWW_VAE_API int pww_vae_attn_fwd(const void *q, const void *k, const void *v, void *o, const pww_vae_attn_desc_t *desc, void *stream) {
    return pww::vae_attn_fwd(q, k, v, o, desc, static_cast<hipStream_t>(stream));
}
PWW_VAE_API size_t pww_vae_tail_workspace_bytes(const pww_vae_tail_desc_t *desc) {
    pww::TailPlan plan;
    return pww::tail_plan(desc, &plan) == PWW_OK ? plan.ws_bytes : 0;
}
PWW_VAE_API int pww_vae_tail_chunks(const pww_vae_tail_desc_t *desc) {
    pww::TailPlan plan;
    return pww::tail_plan(desc, &plan) == PWW_OK ? plan.nchunk : 0;
}
PWW_VAE_API int pww_vae_tail_stats(const void *x, const void *w, const pww_vae_tail_desc_t *desc, void *ws, size_t ws_bytes, void *stream) {
    pww::TailPlan plan;
    return pww::tail_stats(x, w, desc, ws, ws_bytes, static_cast<hipStream_t>(stream), &plan);
}
PWW_VAE_API int pww_vae_tail_fwd(const void *x, const void *gamma, const void *beta, const void *w, const void *bias, void *out,
                                 const pww_vae_tail_desc_t *desc, void *ws, size_t ws_bytes, void *stream) {
    return pww::vae_tail_fwd(x, gamma, beta, w, bias, out, desc, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
