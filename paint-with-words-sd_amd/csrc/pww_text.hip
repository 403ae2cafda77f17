// The three pieces of a CLIP text encoder that have no other kernel here (include/pww_hip_text.h). The encoder is launch-bound: 77 tokens a
// row, two rows for a plain request. Every kernel below is therefore ONE small launch that replaces several stock ones, and none of them is
// tuned past that: the launch itself is the cost.
//
// 1. pww_text_embed_ln: token gather + position add + layer 0's layer_norm1. One wave per token row (four rows per workgroup); the row stays
//    in registers between the add and the LayerNorm (C <= 4096: 64 fp32 per lane), the two reductions are xor butterflies over the wave, so
//    every lane holds the same sums and the result does not depend on anything but the row.
//
// 2. pww_text_attn_fwd: causal self-attention, head dim 64, L <= 128, on MFMA 32 x 32 x 16. Grid (32-query blocks, rows x heads), ONE wave per
//    workgroup. A plain SD1.5 request is 24 (row, head) pairs; with a workgroup per pair the launch would occupy 24 of the 256 CUs and each
//    would walk the three query blocks one after the other. The grid over query blocks gives 72 independent waves, and a causal block reads
//    only the keys up to its own end: block b forms b + 1 score tiles, not 3. K and V of a (row, head) are at most 16 KB each, so the cost
//    of reading them once per query block (from L2 after the first) is small beside a launch.
//      S^T        the K rows are the A operand as they lie in memory (a lane reads 16 bytes of ITS key per step), Q^T is B: lane (q, half)
//                 then holds 16 keys of ONE query per 32-key tile, and a row maximum / sum is 16 registers and one exchange with lane ^ 32.
//                 All of a query's scores (at most 4 tiles x 16) stay in registers: the softmax is the plain one -- maximum, exp, sum,
//                 divide -- in fp32, and the NORMALISED probability is what is rounded to the storage type, as the stock route rounds it.
//      O^T        V^T (LDS) is A, P^T (registers) is B. The product sums over V's ROW index, so V goes through LDS transposed: each lane
//                 loads 8 keys x 8 columns, transposes in registers and stores 8 x 16 bytes into the [column][key slot] image. The key slot
//                 order is the order in which a lane holds its scores (pww_common.h, swap23): slot 16 s + 8 h + j is key
//                 16 s + 8 (j >> 2) + 4 h + (j & 3) of the tile. Rows are 272 bytes: the 16-byte reads of 16 lanes hit 16 bank groups.
//    A key index at or past L is clamped to L - 1 for the load (so no row outside the tensor is read) and masked in the scores; a masked
//    probability is exactly 0.
//
// 3. pww_text_act: QuickGELU / GELU in place, 8 elements per thread, fp32, one rounding.
//
// Built as a library of its own (libpww_hip_text.so): host plumbing from pww_side_host.h, only pww_text_* visible.
#define PWW_SIDE_LIB "libpww_hip_text"
#include "pww_side_host.h"
#include "../../include/pww_hip_text.h"

#include <math.h>

#define PWW_TEXT_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

// ---- embedding + LayerNorm ---------------------------------------------------------------------------------------------------------------
constexpr int TE_THREADS = 256, TE_ROWS = TE_THREADS / 64, TE_MAXV = PWW_TEXT_MAX_WIDTH / 8 / 64;      // 16-byte vectors per lane: 8

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T>
__global__ void __launch_bounds__(TE_THREADS) text_embed_ln_kernel(const int *ids, const T *tok, const T *pos, const T *gamma, const T *beta, T *x, T *h,
                                                                   int rows, int L, int C, int V, float eps) {
    typedef typename Vec<T>::v8 V8;
    const int lane = threadIdx.x & 63, row = blockIdx.x * TE_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;        // (wave-uniform; no workgroup barrier below)
    const int l = row % L, nvec = C >> 3;
    const int id = min(max(ids[row], 0), V - 1);
    const T *tp = tok + (long)id * C, *pp = pos + (long)l * C;
    T *xp = x + (long)row * C, *hp = h + (long)row * C;
    float xv[TE_MAXV][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < TE_MAXV; ++i) {
        const int vi = i * 64 + lane;
        if (vi < nvec) {
            const V8 a = *reinterpret_cast<const V8 *>(tp + 8 * vi), b = *reinterpret_cast<const V8 *>(pp + 8 * vi);
            V8 s;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s[e] = (T)((float)a[e] + (float)b[e]);
                xv[i][e] = (float)s[e];
                sum += xv[i][e];
            }
            *reinterpret_cast<V8 *>(xp + 8 * vi) = s;
        }
    }
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < TE_MAXV; ++i)
        if (i * 64 + lane < nvec) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = xv[i][e] - mean;
                sq += d * d;
            }
        }
    const float rstd = 1.f / sqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < TE_MAXV; ++i) {
        const int vi = i * 64 + lane;
        if (vi < nvec) {
            const V8 g = *reinterpret_cast<const V8 *>(gamma + 8 * vi), b = *reinterpret_cast<const V8 *>(beta + 8 * vi);
            V8 y;
#pragma unroll
            for (int e = 0; e < 8; ++e) y[e] = (T)((xv[i][e] - mean) * rstd * (float)g[e] + (float)b[e]);
            *reinterpret_cast<V8 *>(hp + 8 * vi) = y;
        }
    }
}

// ---- attention ---------------------------------------------------------------------------------------------------------------------------
constexpr int TA_D = PWW_TEXT_HEAD_DIM, TA_BM = 32, TA_MAXKB = PWW_TEXT_MAX_TOKENS / 32;
constexpr int TA_VT_ROW = 2 * PWW_TEXT_MAX_TOKENS + 16;         // 128 key slots of one column + 16 bytes
constexpr int TA_LDS = TA_D * TA_VT_ROW;                        // 17 408

struct TextAttnArgs {
    const void *qkv;
    void *o;
    long ld, old;       // row strides, in elements
    int L, H, C;
    float scale_log2;   // 64^-0.5 * log2(e)
};

template <typename T>
__global__ void __launch_bounds__(64) text_attn_kernel(const TextAttnArgs p) {
    typedef typename Vec<T>::v8 V8;
    typedef typename Vec<T>::v4 V4;
    __shared__ __attribute__((aligned(16))) char vt[TA_LDS];
    const int lane = threadIdx.x, l31 = lane & 31, h = lane >> 5;
    const int qb = blockIdx.x, row = blockIdx.y / p.H, head = blockIdx.y - row * p.H, L = p.L;
    const T *base = reinterpret_cast<const T *>(p.qkv) + (long)row * L * p.ld + head * TA_D;      // q of this (row, head); k at + C, v at + 2 C

    // V^T image of the key tiles 0 .. qb: a lane owns 8 columns (cg) of one 8-slot group (tile bb of the pass, step s, half hh)
    {
        const int cg = lane & 7, oct = lane >> 3, bb = oct >> 2, ss = (oct >> 1) & 1, hh = oct & 1;
#pragma unroll
        for (int pass = 0; pass < TA_MAXKB / 2; ++pass) {
            const int kb = 2 * pass + bb;
            if (kb <= qb) {
                V8 vf[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const int key = min(kb * 32 + 16 * ss + 8 * (jj >> 2) + 4 * hh + (jj & 3), L - 1);
                    vf[jj] = *reinterpret_cast<const V8 *>(base + (long)key * p.ld + 2 * p.C + 8 * cg);
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    V8 t;
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) t[jj] = vf[jj][c];
                    *reinterpret_cast<V8 *>(vt + (8 * cg + c) * TA_VT_ROW + 2 * (kb * 32 + 16 * ss + 8 * hh)) = t;
                }
            }
        }
    }

    // S^T[key][query]: k-slot (st, h, j) is head-dim element 16 st + 8 h + j for K and Q alike
    const int qidx = qb * TA_BM + l31;
    V8 qf[4];
    {
        const T *qp = base + (long)min(qidx, L - 1) * p.ld + 8 * h;
#pragma unroll
        for (int st = 0; st < 4; ++st) qf[st] = *reinterpret_cast<const V8 *>(qp + 16 * st);
    }
    f32x16 s[TA_MAXKB];
#pragma unroll
    for (int kb = 0; kb < TA_MAXKB; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
        if (kb <= qb) {         // (uniform)
            const T *kp = base + (long)min(kb * 32 + l31, L - 1) * p.ld + p.C + 8 * h;
#pragma unroll
            for (int st = 0; st < 4; ++st) s[kb] = mfma32(*reinterpret_cast<const V8 *>(kp + 16 * st), qf[st], s[kb]);
        }
    }
    // the softmax of this lane's query over keys <= the query (key 0 is live for every query: the maximum is finite)
    float m = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < TA_MAXKB; ++kb)
        if (kb <= qb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = (key <= qidx && key < L) ? s[kb][r] * p.scale_log2 : -INFINITY;
                s[kb][r] = v;
                m = fmaxf(m, v);
            }
        }
    m = fmaxf(m, __shfl_xor(m, 32));
    float lsum = 0.f;
#pragma unroll
    for (int kb = 0; kb < TA_MAXKB; ++kb)
        if (kb <= qb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[kb][r] - m);
                s[kb][r] = e;
                lsum += e;
            }
        }
    lsum += __shfl_xor(lsum, 32);
    const float inv = 1.f / lsum;

    __syncthreads();            // the V^T image is complete

    // O^T[column][query] += V^T P^T
    f32x16 oacc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < TA_MAXKB; ++kb)
        if (kb <= qb) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                V8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (T)(s[kb][8 * st + j] * inv);
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    oacc[t] = mfma32(*reinterpret_cast<const V8 *>(vt + (32 * t + l31) * TA_VT_ROW + 2 * (kb * 32 + 16 * st + 8 * h)), pf, oacc[t]);
            }
        }
    if (qidx < L) {
        T *op = reinterpret_cast<T *>(p.o) + ((long)row * L + qidx) * p.old + head * TA_D + 4 * h;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                V4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (T)oacc[t][4 * rq + i];
                *reinterpret_cast<V4 *>(op + 32 * t + 8 * rq) = o;
            }
    }
}

// ---- activation --------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) text_act_kernel(T *x, long nv_total, int nv, long stride, int act) {
    typedef typename Vec<T>::v8 V8;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nv_total) return;
    const long r = idx / nv;
    T *xp = x + r * stride + 8 * (idx - r * nv);
    V8 v = *reinterpret_cast<const V8 *>(xp);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float g = (float)v[e];
        float y;
        if (act == PWW_TEXT_ACT_QUICK_GELU)     // exp2 of a large argument is +inf, its reciprocal 0: the sigmoid saturates, nothing is NaN
            y = g * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.702f * 1.44269504088896341f * g));
        else
            y = 0.5f * g * (1.f + erff(g * 0.70710678118654752440f));
        v[e] = (T)y;
    }
    *reinterpret_cast<V8 *>(xp) = v;
}

bool dtype_ok(int dtype) { return dtype == PWW_DTYPE_F16 || dtype == PWW_DTYPE_BF16; }

}  // namespace

int text_embed_ln(const void *ids, const void *tok, const void *pos, const void *gamma, const void *beta, void *x, void *h, int R, int L, int C, int V, int P,
                  float eps, int dtype, hipStream_t stream) {
    if (!ids || !tok || !pos || !gamma || !beta || !x || !h) { set_error("text_embed_ln: ids, tok, pos, gamma, beta, x and h are required"); return PWW_EINVAL; }
    if (R < 1 || L < 1 || V < 1 || P < 1) { set_error("text_embed_ln: bad argument (R %d L %d V %d P %d): sizes >= 1", R, L, V, P); return PWW_EINVAL; }
    if (!dtype_ok(dtype)) { set_error("text_embed_ln: unsupported dtype %d (F16 / BF16)", dtype); return PWW_ENOTSUP; }
    if (C < 64 || C % 64 != 0 || C > PWW_TEXT_MAX_WIDTH) { set_error("text_embed_ln: C %d must be a multiple of 64, at most %d", C, PWW_TEXT_MAX_WIDTH); return PWW_ENOTSUP; }
    if (L > P) { set_error("text_embed_ln: %d tokens exceed the %d positions of the table", L, P); return PWW_ENOTSUP; }
    if (!(eps > 0.f)) { set_error("text_embed_ln: eps must be > 0"); return PWW_ENOTSUP; }
    if ((int64_t)R * L * C >= ((int64_t)1 << 31)) { set_error("text_embed_ln: tensor of 2^31 elements or more"); return PWW_ENOTSUP; }
    if (!aligned16(tok) || !aligned16(pos) || !aligned16(gamma) || !aligned16(beta) || !aligned16(x) || !aligned16(h) || (reinterpret_cast<uintptr_t>(ids) & 3)) {
        set_error("text_embed_ln: the tables, the affine and the outputs must be 16-byte aligned, ids 4-byte aligned");
        return PWW_ENOTSUP;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    const int rows = R * L;
    const dim3 grid((rows + TE_ROWS - 1) / TE_ROWS), block(TE_THREADS);
    const int *idp = static_cast<const int *>(ids);
    if (dtype == PWW_DTYPE_F16)
        launch_timed(text_embed_ln_kernel<f16>, grid, block, 0, stream, idp, static_cast<const f16 *>(tok), static_cast<const f16 *>(pos), static_cast<const f16 *>(gamma),
                     static_cast<const f16 *>(beta), static_cast<f16 *>(x), static_cast<f16 *>(h), rows, L, C, V, eps);
    else
        launch_timed(text_embed_ln_kernel<bf16>, grid, block, 0, stream, idp, static_cast<const bf16 *>(tok), static_cast<const bf16 *>(pos), static_cast<const bf16 *>(gamma),
                     static_cast<const bf16 *>(beta), static_cast<bf16 *>(x), static_cast<bf16 *>(h), rows, L, C, V, eps);
    return check_hip(hipGetLastError(), "text_embed_ln launch");
}

int text_attn_fwd(const void *qkv, void *o, int R, int H, int L, int64_t ld, int64_t old, int dtype, hipStream_t stream) {
    if (!qkv || !o) { set_error("text_attn: qkv and o are required"); return PWW_EINVAL; }
    if (R < 1 || H < 1 || L < 1) { set_error("text_attn: bad argument (R %d H %d L %d): sizes >= 1", R, H, L); return PWW_EINVAL; }
    if (!dtype_ok(dtype)) { set_error("text_attn: unsupported dtype %d (F16 / BF16)", dtype); return PWW_ENOTSUP; }
    if (L > PWW_TEXT_MAX_TOKENS) { set_error("text_attn: %d tokens, at most %d are supported", L, PWW_TEXT_MAX_TOKENS); return PWW_ENOTSUP; }
    const int64_t C = (int64_t)H * TA_D, lim = (int64_t)1 << 31;
    if (ld < 3 * C || old < C || (ld & 7) || (old & 7)) {
        set_error("text_attn: row strides (qkv %ld, o %ld) must cover 3 C = %ld and C and be multiples of 8 elements", (long)ld, (long)old, (long)(3 * C));
        return PWW_ENOTSUP;
    }
    if ((int64_t)R * H > 65535) { set_error("text_attn: more than 65535 (row, head) pairs"); return PWW_ENOTSUP; }
    if ((int64_t)R * L * ld >= lim || (int64_t)R * L * old >= lim) { set_error("text_attn: extent of 2^31 elements or more"); return PWW_ENOTSUP; }
    if (!aligned16(qkv) || !aligned16(o)) { set_error("text_attn: qkv and o must be 16-byte aligned"); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;
    const TextAttnArgs args{qkv, o, (long)ld, (long)old, L, H, (int)C, 0.125f * 1.44269504088896341f};
    const dim3 grid((L + TA_BM - 1) / TA_BM, R * H), block(64);
    if (dtype == PWW_DTYPE_F16) launch_timed(text_attn_kernel<f16>, grid, block, 0, stream, args);
    else launch_timed(text_attn_kernel<bf16>, grid, block, 0, stream, args);
    return check_hip(hipGetLastError(), "text_attn launch");
}

int text_act(void *x, int64_t M, int N, int64_t stride, int act, int dtype, hipStream_t stream) {
    if (!x) { set_error("text_act: x is required"); return PWW_EINVAL; }
    if (M < 1 || N < 1) { set_error("text_act: bad argument (M %ld N %d): sizes >= 1", (long)M, N); return PWW_EINVAL; }
    if (!dtype_ok(dtype)) { set_error("text_act: unsupported dtype %d (F16 / BF16)", dtype); return PWW_ENOTSUP; }
    if (act != PWW_TEXT_ACT_QUICK_GELU && act != PWW_TEXT_ACT_GELU) { set_error("text_act: unknown activation %d (quick_gelu 0 / gelu 1)", act); return PWW_ENOTSUP; }
    if ((N & 7) || (stride & 7) || stride < N) { set_error("text_act: N %d and the row stride %ld must be multiples of 8 elements, stride >= N", N, (long)stride); return PWW_ENOTSUP; }
    if (M >= ((int64_t)1 << 31) || M * stride >= ((int64_t)1 << 31)) { set_error("text_act: extent of 2^31 elements or more"); return PWW_ENOTSUP; }
    if (!aligned16(x)) { set_error("text_act: x must be 16-byte aligned"); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;
    const int nv = N / 8;
    const long total = (long)M * nv;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (dtype == PWW_DTYPE_F16) launch_timed(text_act_kernel<f16>, grid, block, 0, stream, static_cast<f16 *>(x), total, nv, (long)stride, act);
    else launch_timed(text_act_kernel<bf16>, grid, block, 0, stream, static_cast<bf16 *>(x), total, nv, (long)stride, act);
    return check_hip(hipGetLastError(), "text_act launch");
}

}  // namespace pww

PWW_TEXT_API int pww_text_version(void) { return PWW_TEXT_VERSION; }
PWW_TEXT_API const char *pww_text_last_error(void) { return pww::last_error(); }
PWW_TEXT_API int pww_text_embed_ln(const void *ids, const void *tok, const void *pos, const void *gamma, const void *beta, void *x, void *h, int32_t R, int32_t L,
                                   int32_t C, int32_t V, int32_t P, float eps, int32_t dtype, void *stream) {
    return pww::text_embed_ln(ids, tok, pos, gamma, beta, x, h, R, L, C, V, P, eps, dtype, static_cast<hipStream_t>(stream));
}
PWW_TEXT_API int pww_text_attn_fwd(const void *qkv, void *o, int32_t R, int32_t H, int32_t L, int64_t qkv_stride, int64_t o_stride, int32_t dtype, void *stream) {
    return pww::text_attn_fwd(qkv, o, R, H, L, qkv_stride, o_stride, dtype, static_cast<hipStream_t>(stream));
}
PWW_TEXT_API int pww_text_act(void *x, int64_t M, int32_t N, int64_t stride, int32_t act, int32_t dtype, void *stream) {
    return pww::text_act(x, M, N, stride, act, dtype, static_cast<hipStream_t>(stream));
}
