// Unmerged LoRA adapters chosen per batch row (pww_lora_fwd): behind a linear layer y = x W^T,
//
//   y[r] += s_r * (x[r] A_i^T) B_i^T,     i = row_adapter[r], s_r = row_scale[r],   A_i [rank][K], B_i [N][rank]
//
// in place, one launch for every row, adapter and column segment (the fused q|k|v and k|v projections have one (A, B) pair per segment).
// A merged adapter (W + s B A) applies to every row alike; this one is chosen by two small device arrays the sampler rewrites per request,
// so a captured graph replays with a new assignment.
//
// Work decomposition. Grid (token tiles of 64, segments x column chunks, rows); a 256-thread workgroup is 4 waves of 16 tokens each, and
// the waves never exchange anything: no LDS, no barrier. A workgroup whose row has no adapter (or scale 0) returns after reading the row's
// two scalars. Otherwise each wave
//   1. forms t = x A^T for its 16 tokens and ALL rank columns with mfma_f32_16x16x32 (A_i rows as the A operand, token rows as the B
//      operand, both loaded from global memory in operand layout: 16 bytes per lane and K-step; x is read once per workgroup, A_i comes
//      from L2), rounds t to the storage type once;
//   2. walks its column chunk 32 columns at a time: u = t B^T with the rank as the MFMA's k, then y = T(float(y) + s u) with one 16-byte
//      load and one 16-byte store per lane.
// Between the two products no data moves: step 1 leaves lane (fr, fq) with t[token fr][16 rr + 4 fq + 0..3] of every 16-column tile rr,
// step 2 needs 8 k-values per lane and 32-step. A sum over the rank does not care about the order of its terms as long as both operands
// agree, so k-slot 8 fq + j of step s is DEFINED as rank column 32 s + 4 fq + j (j < 4) and 32 s + 16 + 4 fq + (j - 4) (j >= 4): the t
// operand is two accumulators side by side, and the B_i operand is two 8-byte loads at those columns. In the same way the 16 A-operand rows
// of the second product's two tiles are output columns c + 8 (i >> 2) + (i & 3) and + 4, which leaves each lane with 8 CONSECUTIVE output
// columns of one token.
// The first product is recomputed per column chunk (host: lora_plan): it is the cheap one, and the 64-token levels of the UNet would
// otherwise run on R workgroups.
//
// Built as a library of its own (libpww_hip_lora.so, include/pww_hip_lora.h): host plumbing from pww_side_host.h, only pww_lora_* visible.
#define PWW_SIDE_LIB "libpww_hip_lora"
#include "pww_side_host.h"
#include "../../include/pww_hip_lora.h"

#define PWW_LORA_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int LR_THREADS = 256, LR_BT = 64;     // tokens per workgroup: 16 per wave
constexpr int LR_MIN_CHUNK = 64;                // narrowest column chunk the host plans (a multiple of 32)
constexpr int LR_TARGET_WG = 256;               // column chunks are narrowed until the grid has about one workgroup per CU

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

struct LoraArgs {
    const void *x, *a, *b;
    const int *row_adapter;
    const float *row_scale;
    void *y;
    long xrs, xts, yrs, yts;    // row / token strides of x and y, in elements
    int T, K, n_seg, seg_cols;  // seg_cols = N / n_seg
    int n_adapters, cw, nchunk; // cw = columns per chunk (a multiple of 32), nchunk = chunks per segment
};

template <typename T, int RANK>
__global__ void __launch_bounds__(LR_THREADS) lora_kernel(const LoraArgs p) {
    typedef typename Vec<T>::v8 V8;
    typedef typename Vec<T>::v4 V4;
    constexpr int RT = RANK / 16, RS = RANK / 32;

    const int r = blockIdx.z;
    const int ad = p.row_adapter[r];
    const float s = p.row_scale[r];
    if (ad < 0 || ad >= p.n_adapters || s == 0.f) return;      // (uniform) this row keeps y bit for bit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int tok0 = blockIdx.x * LR_BT + wave * 16;
    if (tok0 >= p.T) return;                                    // (wave-uniform; the waves share nothing)
    const int seg = blockIdx.y / p.nchunk, chunk = blockIdx.y - seg * p.nchunk;
    const int tok = tok0 + fr;
    const bool live = tok < p.T;
    const int tl = live ? tok : p.T - 1;                        // tail lanes load a clamped token row and store nothing

    // 1. t[token fr][rank] = x A^T. Lane (fr, fq) supplies x[tl][k0 + 8 fq ..] and A[16 rr + fr][k0 + 8 fq ..] and receives
    //    D[rank row 16 rr + 4 fq + j][token fr].
    const T *xp = reinterpret_cast<const T *>(p.x) + (long)r * p.xrs + (long)tl * p.xts + fq * 8;
    const T *ap = reinterpret_cast<const T *>(p.a) + ((long)(ad * p.n_seg + seg) * RANK + fr) * p.K + fq * 8;
    f32x4 acc[RT];
#pragma unroll
    for (int rr = 0; rr < RT; ++rr) acc[rr] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += 32) {
        const V8 xf = *reinterpret_cast<const V8 *>(xp + k0);
#pragma unroll
        for (int rr = 0; rr < RT; ++rr) {
            const V8 af = *reinterpret_cast<const V8 *>(ap + (long)rr * 16 * p.K + k0);
            acc[rr] = mfma16(af, xf, acc[rr]);
        }
    }
    // the second product's t operand: k-slot 8 fq + j of step q is rank column 32 q + 4 fq + j (j < 4), 32 q + 16 + 4 fq + j - 4 (j >= 4)
    V8 tf[RS];
#pragma unroll
    for (int q = 0; q < RS; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tf[q][j] = (T)acc[2 * q][j];
            tf[q][4 + j] = (T)acc[2 * q + 1][j];
        }

    // 2. this chunk's columns, 32 at a time. A-operand row i of the two tiles is column c + 8 (i >> 2) + (i & 3) and that + 4, so the lane
    //    receives columns c + 8 fq .. + 7 of token fr. seg_cols is a multiple of 16 and c of 32: a short last step masks fq >= 2.
    const int c_end = min((chunk + 1) * p.cw, p.seg_cols);
    const T *bseg = reinterpret_cast<const T *>(p.b) + (long)(ad * p.n_seg + seg) * p.seg_cols * RANK + 4 * fq;
    T *yp = reinterpret_cast<T *>(p.y) + (long)r * p.yrs + (long)tl * p.yts + (long)seg * p.seg_cols + 8 * fq;
    for (int c = chunk * p.cw; c < c_end; c += 32) {
        const int n0 = min(c + 8 * (fr >> 2) + (fr & 3), p.seg_cols - 5);       // (clamped rows feed columns that are masked below)
        const T *b0 = bseg + (long)n0 * RANK, *b1 = b0 + 4 * RANK;
        f32x4 u0 = f32x4{0.f, 0.f, 0.f, 0.f}, u1 = u0;
#pragma unroll
        for (int q = 0; q < RS; ++q) {
            const V4 l0 = *reinterpret_cast<const V4 *>(b0 + 32 * q), h0 = *reinterpret_cast<const V4 *>(b0 + 32 * q + 16);
            const V4 l1 = *reinterpret_cast<const V4 *>(b1 + 32 * q), h1 = *reinterpret_cast<const V4 *>(b1 + 32 * q + 16);
            u0 = mfma16(__builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7), tf[q], u0);
            u1 = mfma16(__builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7), tf[q], u1);
        }
        if (live && c + 8 * fq + 8 <= c_end) {
            V8 *dst = reinterpret_cast<V8 *>(yp + c);
            V8 o = *dst;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = (T)((float)o[j] + s * u0[j]);
                o[4 + j] = (T)((float)o[4 + j] + s * u1[j]);
            }
            *dst = o;
        }
    }
}

struct LoraPlan { int seg_cols, cw, nchunk, ttiles; };

// PWW_OK, or the code with the error text set. Nothing here touches the HIP runtime.
int lora_plan(const void *x, const void *a, const void *b, const int32_t *row_adapter, const float *row_scale, void *y, const pww_lora_desc_t *d,
              LoraPlan *p) {
    if (!d || d->size < sizeof(pww_lora_desc_t)) { set_error("lora: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    if (!x || !a || !b || !row_adapter || !row_scale || !y) { set_error("lora: x, a, b, row_adapter, row_scale and y are required"); return PWW_EINVAL; }
    if (d->R < 1 || d->T < 1 || d->K < 1 || d->N < 1 || d->n_seg < 1 || d->n_seg > PWW_LORA_MAX_SEGMENTS || d->n_adapters < 1
        || d->n_adapters > PWW_LORA_MAX_ADAPTERS) {
        set_error("lora: bad argument (R %d T %d K %d N %d n_seg %d n_adapters %d): sizes >= 1, 1 .. %d segments, 1 .. %d adapters", d->R, d->T, d->K, d->N,
                  d->n_seg, d->n_adapters, PWW_LORA_MAX_SEGMENTS, PWW_LORA_MAX_ADAPTERS);
        return PWW_EINVAL;
    }
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->rank < 32 || d->rank > PWW_LORA_MAX_RANK || d->rank % 32 != 0 || d->K % 32 != 0
        || d->N % d->n_seg != 0 || (d->N / d->n_seg) % 16 != 0) {
        set_error("lora: unsupported (dtype %d rank %d K %d N %d n_seg %d): rank 32 / 64 / 96 / 128, K a multiple of 32, N / n_seg a multiple of 16", d->dtype,
                  d->rank, d->K, d->N, d->n_seg);
        return PWW_ENOTSUP;
    }
    if (((d->x_row_stride | d->x_tok_stride | d->y_row_stride | d->y_tok_stride) & 7) || d->x_tok_stride < d->K || d->y_tok_stride < d->N
        || d->x_row_stride < (int64_t)d->T * d->x_tok_stride || d->y_row_stride < (int64_t)d->T * d->y_tok_stride) {
        set_error("lora: strides must cover their extents and be multiples of 8 elements (x %ld %ld, y %ld %ld)", (long)d->x_row_stride, (long)d->x_tok_stride,
                  (long)d->y_row_stride, (long)d->y_tok_stride);
        return PWW_ENOTSUP;
    }
    if (!aligned16(x) || !aligned16(a) || !aligned16(b) || !aligned16(y)) { set_error("lora: x, a, b and y must be 16-byte aligned"); return PWW_ENOTSUP; }
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)d->R * d->x_row_stride >= lim || (int64_t)d->R * d->y_row_stride >= lim || (int64_t)d->n_adapters * d->n_seg * d->rank * d->K >= lim
        || (int64_t)d->n_adapters * d->N * d->rank >= lim) {
        set_error("lora: tensor of 2^31 elements or more");
        return PWW_ENOTSUP;
    }
    p->seg_cols = d->N / d->n_seg;
    p->ttiles = (d->T + LR_BT - 1) / LR_BT;
    // column chunks: halve the chunk until the grid has LR_TARGET_WG workgroups or the chunk is LR_MIN_CHUNK wide (the first product is
    // recomputed per chunk)
    int cw = (p->seg_cols + 31) / 32 * 32;
    while ((long)d->R * p->ttiles * d->n_seg * ((p->seg_cols + cw - 1) / cw) < LR_TARGET_WG && cw > LR_MIN_CHUNK) cw = (cw / 2 + 31) / 32 * 32;
    p->cw = cw;
    p->nchunk = (p->seg_cols + cw - 1) / cw;
    return PWW_OK;
}

template <typename T>
int lora_launch(const LoraPlan &p, const pww_lora_desc_t *d, const LoraArgs &args, hipStream_t stream) {
    const dim3 grid(p.ttiles, d->n_seg * p.nchunk, d->R), block(LR_THREADS);
    switch (d->rank) {
    case 32: launch_timed(lora_kernel<T, 32>, grid, block, 0, stream, args); break;
    case 64: launch_timed(lora_kernel<T, 64>, grid, block, 0, stream, args); break;
    case 96: launch_timed(lora_kernel<T, 96>, grid, block, 0, stream, args); break;
    default: launch_timed(lora_kernel<T, 128>, grid, block, 0, stream, args); break;
    }
    return check_hip(hipGetLastError(), "lora launch");
}

}  // namespace

int lora_fwd(const void *x, const void *a, const void *b, const int32_t *row_adapter, const float *row_scale, void *y, const pww_lora_desc_t *d,
             hipStream_t stream) {
    LoraPlan p;
    const int rc = lora_plan(x, a, b, row_adapter, row_scale, y, d, &p);
    if (rc != PWW_OK) return rc;
    if (d->R > 65535 || d->n_seg * p.nchunk > 65535) { set_error("lora: more than 65535 rows or column chunks"); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;
    const LoraArgs args{x, a, b, row_adapter, row_scale, y, d->x_row_stride, d->x_tok_stride, d->y_row_stride, d->y_tok_stride,
                        d->T, d->K, d->n_seg, p.seg_cols, d->n_adapters, p.cw, p.nchunk};
    if (d->dtype == PWW_DTYPE_F16) return lora_launch<f16>(p, d, args, stream);
    return lora_launch<bf16>(p, d, args, stream);
}

}  // namespace pww

PWW_LORA_API int pww_lora_version(void) { return PWW_LORA_VERSION; }
PWW_LORA_API const char *pww_lora_last_error(void) { return pww::last_error(); }
PWW_LORA_API int pww_lora_fwd(const void *x, const void *a, const void *b, const int32_t *row_adapter, const float *row_scale, void *y,
                              const pww_lora_desc_t *desc, void *stream) {
    return pww::lora_fwd(x, a, b, row_adapter, row_scale, y, desc, static_cast<hipStream_t>(stream));
}
