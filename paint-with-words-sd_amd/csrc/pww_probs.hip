// pww_cross_attn_probs: the head-averaged softmax probabilities of one cross-attention call over the prompt tokens,
//     P[b][n][m] = (1 / H) sum_h softmax_m( ((Q K^T)[b,h,n,m] + c[b] bias[b,h,n,m]) scale )
// -- the tensor the reference holds as `attention_scores.softmax(dim=-1)` (paint_with_words/paint_with_words.py:112-114) and every
// attention launch of this library keeps in registers. A diagnostic that runs BESIDE the attention launch of the same call (same q / k /
// map / coefficient inputs), off by default; no attention kernel is touched or shared with it.
//
// One workgroup of four waves owns a 32-row query block of one image. Wave w walks the heads w, w + 4, ...: Q / K fragments straight from
// global memory through buffer descriptors (rows past N / keys past M arrive as zeros), S^T = K Q^T on the 32x32x16 MFMA so that a lane owns
// ONE query row (pww_tile.h), the plain softmax of that row in fp32 (exact maximum, exp, exact sum), and the normalised probabilities added
// into the wave's registers, heads in ascending order. The four partial sums meet in LDS in a fixed order -- waves 0 / 1 store, waves 2 / 3
// add to them, every thread adds the two tiles -- and the block is written with the keys on the lane axis: 16 bytes per lane, a row's M
// floats contiguous across lanes. One owner per output element, no atomics: accumulate = 1 is that owner's read-modify-write, and two
// identical calls give identical bits.
#include "pww_attn_core.h"
#include "pww_cross_tile.h"

namespace pww {

constexpr int PROBS_NW = 4;           // waves per workgroup: the heads are dealt round-robin to them
constexpr int PROBS_KB = 4;           // 32-key blocks at most (M <= 128)
constexpr int PROBS_STRIDE = 132;     // floats per LDS tile row: 128 keys + 4 (a lane's 16-byte pieces of consecutive rows fall into different banks)

struct ProbsParams {
    const void *q, *k;
    const float *bias;                // null: plain softmax
    const double *stats;              // [B][4] or null (stat_kind == PWW_STAT_NONE)
    const float *gate;                // [B] or null
    const float *coeff_scalar_dev;    // replaces coeff_scalar when the kernel runs, or null
    float *out;
    int H, N, M, D;
    long q_sb, q_sh, q_sn;
    long k_sb, k_sh, k_sm;
    long b_sb, b_sh, b_sn, b_sm;
    long o_sb, o_sn;
    float scale, coeff_scalar, weight;
    int stat_kind, accumulate;
    double stat_count;
};

template <typename T>
__global__ void __launch_bounds__(PROBS_NW * 64) probs_kernel(const ProbsParams p) {
    typedef typename Vec<T>::v8 V8;
    __shared__ __attribute__((aligned(16))) float tile[2][32 * PROBS_STRIDE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, l31 = lane & 31;
    const int rb = blockIdx.x, b = blockIdx.y;
    const int qrow = rb * 32 + l31;

    // c[b] = coeff_scalar * stat(stats[b]) * gate[b], fp32 products in this order: the attention launch's coefficient (pww_attn_core.h
    // bias_coefficient; pww_cross_lean.hip / pww_cross_kernel.h form the same products from the statistics they fold and hand out)
    float coeff = 0.f;
    if (p.bias) {
        const float gate = p.gate ? p.gate[b] : 1.f;
        if (gate != 0.f) {                            // (a gated-out image's statistics may never have been written)
            coeff = p.coeff_scalar_dev ? *p.coeff_scalar_dev : p.coeff_scalar;
            if (p.stat_kind != PWW_STAT_NONE) coeff = stat_coefficient(coeff, p.stat_kind, p.stats + (long)b * 4, p.stat_count);
            if (p.gate) coeff = coeff * gate;
        }
    }

    float acc[PROBS_KB][16];
#pragma unroll
    for (int kb = 0; kb < PROBS_KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kb][r] = 0.f;

    const unsigned q_off = (unsigned)((long)qrow * p.q_sn * 2);
    const unsigned k_lane = (unsigned)((long)swap23(l31) * p.k_sm * 2), k_blk = (unsigned)(32 * p.k_sm * 2);
    const unsigned b_row = (unsigned)((long)qrow * p.b_sn * 4);
    const bool b_unit = p.b_sm == 1;
    const float c2 = p.scale * 1.44269504088896340736f;      // the exponentials run as exp2: t = (s + c * bias) * (scale * log2 e)
    const int nks = (p.D + 15) >> 4;                  // 16-wide contraction steps, a RUN-TIME bound: one instantiation per storage type serves every head dim
    const unsigned d_lane = (unsigned)hi * 16u;       // byte offset of the lane's half of a step
    const bool d_tail = (p.D & 8) != 0;               // the last step's upper half lies past D

    for (int h = wave; h < p.H; h += PROBS_NW) {      // (wave-uniform trip count)
        const T *Qp = reinterpret_cast<const T *>(p.q) + b * p.q_sb + h * p.q_sh;
        const T *Kp = reinterpret_cast<const T *>(p.k) + b * p.k_sb + h * p.k_sh;
        const auto srd_q = head_srd(Qp, p.N, p.q_sn, p.D);
        const auto srd_k = head_srd(Kp, p.M, p.k_sm, p.D);
        // register r of block kb = key kb * 32 + 16 (r >> 3) + 8 hi + (r & 7) of the lane's row. Per contraction step a lane moves ONE 16-byte
        // piece of its Q row and one of a K row per key block; the next step's five pieces are in flight under this step's four MFMAs. Rows
        // past N, key blocks past M and the half step past D lie beyond the descriptors (or get an out-of-range offset): zeros, whose
        // products leave the fp32 sums alone -- no branch per MFMA.
        f32x16 s[PROBS_KB];
#pragma unroll
        for (int kb = 0; kb < PROBS_KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
        u32x4 cur[1 + PROBS_KB], nxt[1 + PROBS_KB];
        auto request = [&](u32x4 (&f)[1 + PROBS_KB], int ks) {
            const bool live = ks < nks && !(d_tail && hi && ks == nks - 1);
            const unsigned d_off = (unsigned)ks * 32u + d_lane;
            f[0] = __builtin_amdgcn_raw_buffer_load_b128(srd_q, live ? q_off + d_off : OOB_OFF, 0, 0);
#pragma unroll
            for (int kb = 0; kb < PROBS_KB; ++kb)
                f[1 + kb] = __builtin_amdgcn_raw_buffer_load_b128(srd_k, live ? k_lane + (unsigned)kb * k_blk + d_off : OOB_OFF, 0, 0);
        };
        request(cur, 0);
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
            request(nxt, ks + 1);
#pragma unroll
            for (int kb = 0; kb < PROBS_KB; ++kb) s[kb] = mfma32(__builtin_bit_cast(V8, cur[1 + kb]), __builtin_bit_cast(V8, cur[0]), s[kb]);
#pragma unroll
            for (int i = 0; i < 1 + PROBS_KB; ++i) cur[i] = nxt[i];
        }
        if (p.bias) {
            const float *bbase = p.bias + b * p.b_sb + h * p.b_sh;
            const unsigned bytes = (unsigned)(((long)(p.N - 1) * p.b_sn + (long)(p.M - 1) * p.b_sm + 1) * 4);
            const auto srd_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(bbase), 0, bytes, 0x00020000);
            if (b_unit) {       // (uniform) a lane's 8 consecutive keys are 32 contiguous bytes of its bias row (the [N, 77] maps)
#pragma unroll
                for (int kb = 0; kb < PROBS_KB; ++kb) {
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        const unsigned off = b_row + (unsigned)(kb * 32 + 16 * g + 8 * hi) * 4u;
                        const u32x4 b0 = __builtin_amdgcn_raw_buffer_load_b128(srd_b, off, 0, 0);
                        const u32x4 b1 = __builtin_amdgcn_raw_buffer_load_b128(srd_b, off + 16u, 0, 0);
#pragma unroll
                        for (int j = 0; j < 8; ++j) s[kb][g * 8 + j] = fmaf(__builtin_bit_cast(float, j < 4 ? b0[j] : b1[j - 4]), coeff, s[kb][g * 8 + j]);
                    }
                }
            } else {
                unsigned kstep = (unsigned)(p.b_sm * 4);
                asm volatile("" : "+v"(kstep));       // (opaque: the 64 products key * stride of this rare form are formed where they are used)
#pragma unroll
                for (int kb = 0; kb < PROBS_KB; ++kb) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned off = b_row + (unsigned)(key_of(0, r, hi) + kb * 32) * kstep;
                        s[kb][r] = fmaf(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_b, off, 0, 0)), coeff, s[kb][r]);
                    }
                }
            }
        }
        // keys past M leave the softmax (that includes whole key blocks past M: exp2(-inf) = 0)
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < PROBS_KB; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t = key_of(0, r, hi) + kb * 32 < p.M ? s[kb][r] * c2 : -INFINITY;
                s[kb][r] = t;
                mx = fmaxf(mx, t);
            }
        }
        mx = xhalf_max(mx);                           // finite: key 0 of the row is live
        float l = 0.f;
#pragma unroll
        for (int kb = 0; kb < PROBS_KB; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[kb][r] - mx);
                s[kb][r] = e;
                l += e;
            }
        }
        l += __shfl_xor(l, 32);
        const float inv = 1.f / l;
#pragma unroll
        for (int kb = 0; kb < PROBS_KB; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kb][r] = fmaf(s[kb][r], inv, acc[kb][r]);
        }
    }

    // ---- the four waves' sums meet in LDS, fixed order: (w0 + w2) + (w1 + w3). Every wave addresses the tile alike (lane -> row l31,
    // 8 consecutive keys per piece), so waves 2 / 3 add to exactly the words waves 0 / 1 wrote.
    float *mine = tile[wave & 1] + l31 * PROBS_STRIDE + 8 * hi;
    if (wave < 2) {
#pragma unroll
        for (int kb = 0; kb < PROBS_KB; ++kb) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<f32x4 *>(mine + kb * 32 + 16 * (g >> 1) + 4 * (g & 1)) =
                    f32x4{acc[kb][g * 4], acc[kb][g * 4 + 1], acc[kb][g * 4 + 2], acc[kb][g * 4 + 3]};
        }
    }
    __syncthreads();
    if (wave >= 2) {
#pragma unroll
        for (int kb = 0; kb < PROBS_KB; ++kb) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 *w = reinterpret_cast<f32x4 *>(mine + kb * 32 + 16 * (g >> 1) + 4 * (g & 1));
                const f32x4 v = *w;
                *w = f32x4{v[0] + acc[kb][g * 4], v[1] + acc[kb][g * 4 + 1], v[2] + acc[kb][g * 4 + 2], v[3] + acc[kb][g * 4 + 3]};
            }
        }
    }
    __syncthreads();

    // ---- store: thread -> (row t >> 5 of a pass of 8 rows, keys 4 (t & 31) .. + 3)
    const int c4 = threadIdx.x & 31, key0 = c4 * 4;
    const float hf = (float)p.H;
    if (key0 < p.M) {
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int r = (threadIdx.x >> 5) + 8 * i, n = rb * 32 + r;
            if (n < p.N) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(tile[0] + r * PROBS_STRIDE + key0);
                const f32x4 c = *reinterpret_cast<const f32x4 *>(tile[1] + r * PROBS_STRIDE + key0);
                float *dst = p.out + b * p.o_sb + n * p.o_sn + key0;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = p.weight * ((a[j] + c[j]) / hf);
                if (key0 + 3 < p.M) {
                    if (p.accumulate) {
                        const f32x4 old = *reinterpret_cast<const f32x4 *>(dst);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] += old[j];
                    }
                    *reinterpret_cast<f32x4 *>(dst) = v;
                } else {                              // the row's last, partial piece: element by element, nothing past column M - 1 is touched
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (key0 + j < p.M) dst[j] = p.accumulate ? dst[j] + v[j] : v[j];
                }
            }
        }
    }
}

static int probs_fail(int rc, const char *msg) { set_error("pww_cross_attn_probs: %s", msg); return rc; }

}  // namespace pww

extern "C" int pww_cross_attn_probs(const void *q, const void *k, const float *bias, const double *stats, int32_t stat_kind, double stat_count,
                                    float coeff_scalar, const float *gate, const pww_attn_desc_t *d, const pww_cross_opts_t *opts, float *out,
                                    const pww_probs_desc_t *pd, void *stream) {
    using namespace pww;
    // ---- everything that can be said without a device comes first
    if (!q || !k || !d || !out || !pd) return probs_fail(PWW_EINVAL, "null argument (q, k, desc, out, pdesc)");
    if (pd->size < sizeof(pww_probs_desc_t)) {
        set_error("pww_cross_attn_probs: pww_probs_desc_t.size = %u, this library needs %zu", pd->size, sizeof(pww_probs_desc_t));
        return PWW_EINVAL;
    }
    const float *coeff_dev = nullptr;
    if (opts) {
        if (opts->size < 16) { set_error("pww_cross_attn_probs: pww_cross_opts_t.size = %u is not a known layout", opts->size); return PWW_EINVAL; }
        coeff_dev = opts->coeff_scalar_dev;
    }
    if (d->B <= 0 || d->H <= 0 || d->N <= 0 || d->M <= 0 || d->D <= 0) return probs_fail(PWW_EINVAL, "empty problem");
    if (stat_kind < PWW_STAT_NONE || stat_kind > PWW_STAT_ABSMAX) return probs_fail(PWW_EINVAL, "bad statistic selector");
    if (stat_kind != PWW_STAT_NONE && !stats) return probs_fail(PWW_EINVAL, "null stats with a statistic selected");
    if (pd->images < 0 || pd->images > d->B) return probs_fail(PWW_EINVAL, "images must be 0 (all) or at most B");
    if (pd->accumulate != 0 && pd->accumulate != 1) return probs_fail(PWW_EINVAL, "accumulate must be 0 or 1");
    if (d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) return probs_fail(PWW_ENOTSUP, "dtype unsupported");
    if (d->M > 32 * PROBS_KB || d->D % 8 || d->D > PWW_MAX_HEAD_DIM) {
        set_error("pww_cross_attn_probs: unsupported problem (M=%d D=%d; M <= %d, D a multiple of 8, <= %d)", d->M, d->D, 32 * PROBS_KB, PWW_MAX_HEAD_DIM);
        return PWW_ENOTSUP;
    }
    if ((reinterpret_cast<uintptr_t>(q) & 15) || (reinterpret_cast<uintptr_t>(k) & 15) || (reinterpret_cast<uintptr_t>(out) & 15) ||
        (reinterpret_cast<uintptr_t>(bias) & 3) || (reinterpret_cast<uintptr_t>(stats) & 7) || (reinterpret_cast<uintptr_t>(gate) & 3) ||
        (reinterpret_cast<uintptr_t>(coeff_dev) & 3))
        return probs_fail(PWW_EINVAL, "q, k and out must be 16-byte aligned, bias / gate 4-byte, stats 8-byte");
    for (int i = 0; i < 3; ++i)
        if (d->q_stride[i] % 8 || d->k_stride[i] % 8 || d->q_stride[i] < 0 || d->k_stride[i] < 0) return probs_fail(PWW_EINVAL, "q / k strides must be non-negative multiples of 8 elements");
    if (d->q_stride[2] < d->D || d->k_stride[2] < d->D) return probs_fail(PWW_EINVAL, "q / k rows overlap (row stride < D)");
    if (pd->out_stride[1] < d->M || pd->out_stride[1] % 4 || pd->out_stride[0] % 4 || pd->out_stride[0] < 0)
        return probs_fail(PWW_EINVAL, "out row stride must be >= M and, like the image stride, a multiple of 4 floats");
    if (bias)
        for (int i = 0; i < 4; ++i)
            if (d->bias_stride[i] < 0) return probs_fail(PWW_EINVAL, "negative bias stride");
    // (the kernel forms 32-bit byte offsets of rows just past N before the descriptors cut them off)
    if (((long)(d->N + 32) * d->q_stride[2] + d->D) * 2 >= (1L << 31) || ((long)(32 * PROBS_KB + 32) * d->k_stride[2] + d->D) * 2 >= (1L << 31) ||
        (bias && ((long)(d->N + 32) * d->bias_stride[2] + (long)(d->M + 32) * d->bias_stride[3] + 1) * 4 >= (1L << 31)))
        return probs_fail(PWW_ENOTSUP, "one (image, head) slice of q / k / bias must stay below 2 GiB");
    const int images = pd->images ? pd->images : d->B;
    const long nrb = ((long)d->N + 31) / 32;
    if (images > 65535) return probs_fail(PWW_ENOTSUP, "more than 65535 images");
    if (!arch_ok()) return PWW_ENOTSUP;

    ProbsParams p;
    p.q = q; p.k = k; p.bias = bias; p.stats = stats; p.gate = gate; p.coeff_scalar_dev = coeff_dev; p.out = out;
    p.H = d->H; p.N = d->N; p.M = d->M; p.D = d->D;
    p.q_sb = d->q_stride[0]; p.q_sh = d->q_stride[1]; p.q_sn = d->q_stride[2];
    p.k_sb = d->k_stride[0]; p.k_sh = d->k_stride[1]; p.k_sm = d->k_stride[2];
    p.b_sb = bias ? d->bias_stride[0] : 0; p.b_sh = bias ? d->bias_stride[1] : 0; p.b_sn = bias ? d->bias_stride[2] : 0; p.b_sm = bias ? d->bias_stride[3] : 0;
    p.o_sb = pd->out_stride[0]; p.o_sn = pd->out_stride[1];
    p.scale = d->scale; p.coeff_scalar = coeff_scalar; p.weight = pd->weight;
    p.stat_kind = stat_kind; p.accumulate = pd->accumulate; p.stat_count = stat_count;
    const dim3 grid((unsigned)nrb, (unsigned)images), block(PROBS_NW * 64);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // two instantiations, one per storage type: head dim and key count are run-time bounds (the library's size limit leaves room for no more)
    if (d->dtype == PWW_DTYPE_F16) launch_attn_kernel(probs_kernel<f16>, grid, block, 0, st, p);
    else launch_attn_kernel(probs_kernel<bf16>, grid, block, 0, st, p);
    return check_hip(hipGetLastError(), "probs_kernel launch");
}
