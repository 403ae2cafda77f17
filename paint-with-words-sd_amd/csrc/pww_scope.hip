// libpww_hip_scope.so (include/pww_hip_scope.h): cross-attention over the prompt tokens (M <= 128) whose bias coefficient is a statistic of the
// raw scores PER HEAD or PER QUERY ROW -- weight functions such as c * w * g(sigma) * qk.amax(dim=(1, 2), keepdim=True) or
// c * w * g(sigma) * qk.std(dim=-1, keepdim=True).
//
//   scope_head_parts_kernel   partials of the score statistic per (image, head) over a finished Q: qk_parts_kernel's coarse form of
//                             pww_cross_lean.hip (a wave forms the scores of 32 rows against every 32-key block straight from global
//                             memory, the four waves of a workgroup meet in LDS, one partial per workgroup), in a head-major layout.
//   scope_attn_kernel         O = softmax((Q K^T + c w) scale) V, one workgroup per (128 query rows, head, image) like cross_lean_kernel:
//                             every global load of the workgroup is issued before anything is waited for, K / V are parked in LDS once
//                             (rows past M arrive as out-of-range zeros), ONE barrier. Then it differs: a wave forms the scores of ALL
//                             (at most four) 32-key blocks of its 32 rows first -- 64 accumulator registers -- so that
//                               ROW scope:  the statistic of a row is a reduction over the lane's registers and one shuffle across the two
//                                           half-waves: no pre-pass, no partials;
//                               HEAD scope: every wave folds its own head's partials at entry (pww_cross_tile.h, shuffles only);
//                             and the softmax is one-shot (exact row maximum, exp2, row sum) -- nothing to rescale.
//                             The bias row of a lane is read from global memory where the lane needs it (8 consecutive keys = two
//                             16-byte buffer loads per 16-key group), requested before the statistic is reduced.
//
// The host helpers pww_common.h declares are this library's own (pww_side_host.h): nothing is shared with libpww_hip.so at link time,
// and only the pww_scope_* entry points are visible (the unit is compiled with -fvisibility=hidden).
#define PWW_SIDE_LIB "libpww_hip_scope"
#include "pww_side_host.h"
#include "pww_attn_core.h"
#include "pww_cross_tile.h"
#include "../../include/pww_hip_scope.h"

#define PWW_SCOPE_API extern "C" __attribute__((visibility("default")))

namespace pww {

constexpr int SCOPE_NW = 4;               // waves per workgroup, 32 query rows each
constexpr int SCOPE_KB = 4;               // 32-key blocks at most (M <= 128)
constexpr int SCOPE_MAX_PARTS = 256;      // partials per (image, head) the consumer folds from its prologue's load batch

// ------------------------------------------------------------------------------------------------------------------------------------
// head scope: partials per (image, head)
// ------------------------------------------------------------------------------------------------------------------------------------
struct HeadPartsParams {
    const void *q, *k;
    const float *gate;        // [B] or null
    double *partials;         // [B][H][P][4]
    long q_sb, q_sh, q_sn, k_sb, k_sh, k_sm;
    int H, N, M, D;
    int P;                    // partials per (image, head) = gridDim.x
    int rpw;                  // 32-row blocks a wave walks (1 up to N = 32768)
    int fields;               // bit 0 max, 1 min, 2 sum, 3 sum of squares
};

template <typename T, int KS>
__global__ void __launch_bounds__(SCOPE_NW * 64) scope_head_parts_kernel(const HeadPartsParams p) {
    typedef typename Vec<T>::v8 V8;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z, h = blockIdx.y;
    const T *Qp = reinterpret_cast<const T *>(p.q) + (long)b * p.q_sb + (long)h * p.q_sh;
    const T *Kp = reinterpret_cast<const T *>(p.k) + (long)b * p.k_sb + (long)h * p.k_sh;
    const auto srd_q = head_srd(Qp, p.N, p.q_sn, p.D);
    const auto srd_k = head_srd(Kp, p.M, p.k_sm, p.D);
    const int nkb = (p.M + 31) >> 5;
    const unsigned k_lane = (unsigned)((long)swap23(l31) * p.k_sm * 2), k_blk = (unsigned)(32 * p.k_sm * 2);
    if (p.gate && p.gate[b] == 0.f) return;      // a gated-out image: no scores are formed, its rows of `partials` are left untouched (workgroup-uniform, in front of the barrier)
    float vmax = -INFINITY, vmin = INFINITY;
    double dsum = 0.0, dsq = 0.0;
    for (int j = 0; j < p.rpw; ++j) {
        const int qrow = (((int)blockIdx.x * SCOPE_NW + wave) * p.rpw + j) * 32 + l31;
        const bool rvalid = qrow < p.N;
        // rows past N / keys past M lie beyond the descriptors: zeros, no memory traffic
        V8 qf[KS];
        load_q_frags_buf<T, KS>(qf, srd_q, rvalid ? (unsigned)((long)qrow * p.q_sn * 2) : OOB_OFF, hi, p.D);
#pragma unroll 1
        for (int kb = 0; kb < nkb; ++kb) {
            V8 kf[KS];
            load_q_frags_buf<T, KS>(kf, srd_k, k_lane + (unsigned)kb * k_blk, hi, p.D);
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s = mfma32(kf[ks], qf[ks], s);
            // register r = key kb * 32 + 16 (r >> 3) + 8 hi + (r & 7) of row qrow; scores of padding rows / keys are exactly 0: they leave
            // the sums alone, the extremes select them out
            float usum = 0.f, usq = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool live = rvalid && kb * 32 + key_of(0, r, hi) < p.M;
                const float x = s[r];
                vmax = fmaxf(vmax, live ? x : -INFINITY);
                vmin = fminf(vmin, live ? x : INFINITY);
                usum += x;
                usq = fmaf(x, x, usq);
            }
            dsum += (double)usum;
            dsq += (double)usq;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        vmax = fmaxf(vmax, __shfl_xor(vmax, off));
        vmin = fminf(vmin, __shfl_xor(vmin, off));
        dsum += __shfl_xor(dsum, off);
        dsq += __shfl_xor(dsq, off);
    }
    __shared__ double red[SCOPE_NW][4];
    if (lane == 0) { red[wave][0] = (double)vmax; red[wave][1] = (double)vmin; red[wave][2] = dsum; red[wave][3] = dsq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = red[0][0], n = red[0][1], su = red[0][2], sq = red[0][3];
        for (int w = 1; w < SCOPE_NW; ++w) { m = fmax(m, red[w][0]); n = fmin(n, red[w][1]); su += red[w][2]; sq += red[w][3]; }
        double *out = p.partials + (((long)b * p.H + h) * p.P + blockIdx.x) * 4;
        out[0] = (p.fields & 1) ? m : -INFINITY;
        out[1] = (p.fields & 2) ? n : INFINITY;
        out[2] = (p.fields & 4) ? su : 0.0;
        out[3] = (p.fields & 8) ? sq : 0.0;
    }
}

static bool scope_shape_ok(const pww_attn_desc_t *d) {
    return d->M >= 1 && d->M <= PWW_SCOPE_MAX_KEYS && d->D >= 8 && d->D % 8 == 0 && d->D <= PWW_MAX_HEAD_DIM;
}

// 32-row blocks a wave of the partials launch walks, and the partials per (image, head) that gives
static int head_parts_rpw(const pww_attn_desc_t *d) {
    const long nrb = ((long)d->N + 31) / 32;
    return (int)((nrb + (long)SCOPE_NW * SCOPE_MAX_PARTS - 1) / ((long)SCOPE_NW * SCOPE_MAX_PARTS));
}

static int head_parts_count(const pww_attn_desc_t *d) {
    if (!d || d->B <= 0 || d->H <= 0 || d->N <= 0 || !scope_shape_ok(d)) return 0;
    const long nrb = ((long)d->N + 31) / 32, per = (long)SCOPE_NW * head_parts_rpw(d);
    return (int)((nrb + per - 1) / per);
}

// the fields of ONE statistic: this library takes neither PWW_STAT_NONE nor PWW_STAT_ALL (the selector is checked before stat_fields sees it)
static int stat_fields_one(int stat_kind) { return stat_kind == PWW_STAT_NONE || stat_kind == PWW_STAT_ALL ? -1 : stat_fields(stat_kind); }

// what both entry points ask of the descriptor's q / k side
static int check_qk(const char *me, const pww_attn_desc_t *d) {
    if (d->B <= 0 || d->H <= 0 || d->N <= 0 || d->M <= 0 || d->D <= 0) { set_error("%s: non-positive dimension (B=%d H=%d N=%d M=%d D=%d)", me, d->B, d->H, d->N, d->M, d->D); return PWW_EINVAL; }
    if (!scope_shape_ok(d)) {
        set_error("%s: unsupported problem (M=%d D=%d; M <= %d, D a multiple of 8, <= %d)", me, d->M, d->D, PWW_SCOPE_MAX_KEYS, PWW_MAX_HEAD_DIM);
        return PWW_ENOTSUP;
    }
    if (d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) { set_error("%s: dtype %d unsupported", me, d->dtype); return PWW_ENOTSUP; }
    for (int i = 0; i < 3; ++i)
        if (d->q_stride[i] % 8 || d->k_stride[i] % 8 || d->q_stride[i] < 0 || d->k_stride[i] < 0) { set_error("%s: q / k strides must be non-negative multiples of 8 elements", me); return PWW_EINVAL; }
    if (d->q_stride[2] < d->D || d->k_stride[2] < d->D) { set_error("%s: rows overlap (row stride < D)", me); return PWW_EINVAL; }
    // (the kernels form 32-bit byte offsets of rows just past N / M before the descriptors cut them off)
    if (((long)d->N + 4096) * d->q_stride[2] * 2 >= (1L << 31) || ((long)(2 * PWW_SCOPE_MAX_KEYS) * d->k_stride[2] + d->D) * 2 >= (1L << 31)) {
        set_error("%s: one (image, head) slice of q / k must stay below 2 GiB", me);
        return PWW_ENOTSUP;
    }
    if (d->H > 65535 || d->B > 65535) { set_error("%s: more than 65535 heads or images", me); return PWW_ENOTSUP; }
    return PWW_OK;
}

static int scope_head_parts(const void *q, const void *k, const float *gate, const pww_attn_desc_t *d, int stat_kind, double *partials,
                            size_t partials_bytes, hipStream_t stream) {
    const char *me = "pww_scope_head_parts";
    if (!q || !k || !d || !partials) { set_error("%s: null argument", me); return PWW_EINVAL; }
    if (int rc = check_qk(me, d)) return rc;
    const int fields = stat_fields_one(stat_kind);
    if (fields <= 0) { set_error("%s: bad statistic selector %d", me, stat_kind); return PWW_EINVAL; }
    if (!aligned16(q) || !aligned16(k) || !aligned16(partials) || (reinterpret_cast<uintptr_t>(gate) & 3)) {
        set_error("%s: q, k and partials must be 16-byte aligned, gate 4-byte", me);
        return PWW_EINVAL;
    }
    const int P = head_parts_count(d);
    const size_t need = (size_t)d->B * d->H * P * 4 * sizeof(double);
    if (partials_bytes < need) { set_error("%s: partials buffer too small (need %zu bytes)", me, need); return PWW_EINVAL; }
    if (!arch_ok()) return PWW_ENOTSUP;
    HeadPartsParams p;
    p.q = q; p.k = k; p.gate = gate; p.partials = partials;
    p.q_sb = d->q_stride[0]; p.q_sh = d->q_stride[1]; p.q_sn = d->q_stride[2];
    p.k_sb = d->k_stride[0]; p.k_sh = d->k_stride[1]; p.k_sm = d->k_stride[2];
    p.H = d->H; p.N = d->N; p.M = d->M; p.D = d->D;
    p.P = P; p.rpw = head_parts_rpw(d); p.fields = fields;
    const dim3 grid((unsigned)P, (unsigned)d->H, (unsigned)d->B);
#define PWW_SHP(T)                                                                                               \
    do {                                                                                                         \
        const int ks = (d->D + 15) / 16;                                                                         \
        if (ks <= 3) launch_attn_kernel(scope_head_parts_kernel<T, 3>, grid, dim3(SCOPE_NW * 64), 0, stream, p);      \
        else if (ks == 4) launch_attn_kernel(scope_head_parts_kernel<T, 4>, grid, dim3(SCOPE_NW * 64), 0, stream, p); \
        else if (ks == 5) launch_attn_kernel(scope_head_parts_kernel<T, 5>, grid, dim3(SCOPE_NW * 64), 0, stream, p); \
        else if (ks == 6) launch_attn_kernel(scope_head_parts_kernel<T, 6>, grid, dim3(SCOPE_NW * 64), 0, stream, p); \
        else if (ks <= 8) launch_attn_kernel(scope_head_parts_kernel<T, 8>, grid, dim3(SCOPE_NW * 64), 0, stream, p); \
        else launch_attn_kernel(scope_head_parts_kernel<T, 10>, grid, dim3(SCOPE_NW * 64), 0, stream, p);             \
    } while (0)
    if (d->dtype == PWW_DTYPE_F16) PWW_SHP(f16); else PWW_SHP(bf16);
#undef PWW_SHP
    return check_hip(hipGetLastError(), "scope_head_parts_kernel launch");
}

// ------------------------------------------------------------------------------------------------------------------------------------
// the attention launch
// ------------------------------------------------------------------------------------------------------------------------------------
struct ScopeParams {
    AttnParams a;             // a.bias_coeff = the row gate [B] (or null)
    const double *parts;      // HEAD: [B][H][nparts][4]
    int nparts;
    double *stats_out;        // HEAD, optional: [B][H][4]
    int scope;                // PWW_SCOPE_HEAD / PWW_SCOPE_ROW
    int rows;                 // key rows the LDS image holds: M rounded up to whole 32-key blocks
};

template <int KS, int DT> struct ScopeGeom {
    static constexpr int ROW_BYTES = KTile<KS>::STRIDE + VTile<DT>::STRIDE;       // LDS bytes per key row: [K rows][V rows]
    static constexpr size_t MAX_LDS = (size_t)PWW_SCOPE_MAX_KEYS * ROW_BYTES;
};

template <typename T, int KS, int DT>
__global__ void __launch_bounds__(SCOPE_NW * 64, (DT >= 4 ? 1 : 2)) scope_attn_kernel(const ScopeParams sp) {
    typedef typename Vec<T>::v8 V8;
    typedef KTile<KS> KT;
    typedef VTile<DT> VT;
    constexpr int NT = SCOPE_NW * 64, ROWS = PWW_SCOPE_MAX_KEYS;
    constexpr int KRPP = NT / KT::CHK, VRPP = NT / VT::CHK;                   // key rows a pass of the workgroup covers
    constexpr int KPASS = (ROWS + KRPP - 1) / KRPP, VPASS = (ROWS + VRPP - 1) / VRPP;
    const AttnParams &p = sp.a;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *Kl = smem, *Vl = smem + sp.rows * KT::STRIDE;      // (row-linear: key row r of K at r * KT::STRIDE, of V at r * VT::STRIDE)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, l31 = lane & 31;
    const int qb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int nkb = sp.rows >> 5;                             // live 32-key blocks (1 .. 4)
    const bool head = sp.scope == PWW_SCOPE_HEAD;

    // ---- every global load of the workgroup, before anything is waited for: gate, partials, Q fragments, K / V chunks
    const float gate = p.bias_coeff ? p.bias_coeff[b] : 1.f;
    const float c0 = coeff_scalar_of(p);
    const PartsWant want(p.stat_kind, false);
    PartsRegs pregs;
    parts_request(pregs, sp.parts, sp.nparts, b * p.H + h, head, want, lane);
    const T *Qp = reinterpret_cast<const T *>(p.q) + b * p.q_sb + h * p.q_sh;
    const T *Kp = reinterpret_cast<const T *>(p.k) + b * p.k_sb + h * p.k_sh;
    const T *Vp = reinterpret_cast<const T *>(p.v) + b * p.v_sb + h * p.v_sh;
    T *Op = reinterpret_cast<T *>(p.o) + b * p.o_sb + h * p.o_sh;
    const int qrow = (qb * SCOPE_NW + wave) * 32 + l31;
    const bool qvalid = qrow < p.N;
    V8 qf[KS];
    const auto srd_q = head_srd(Qp, p.N, p.q_sn, p.D);
    load_q_frags_buf<T, KS>(qf, srd_q, qvalid ? (unsigned)((long)qrow * p.q_sn * 2) : OOB_OFF, hi, p.D);

    // K / V: thread -> (row kr of a pass, 16-byte column kc); pass i = rows i * KRPP .. of the head. Rows past M, the head-dim padding
    // and idle threads are out of range of the descriptor: zeros, no memory traffic
    u32x4 kreg[KPASS], vreg[VPASS];
    const int kr = tid / KT::CHK, kc = tid - kr * KT::CHK;
    const int vr = tid / VT::CHK, vc = tid - vr * VT::CHK;
    const bool k_act = kr < KRPP, v_act = vr < VRPP;
    {
        const auto srd_k = head_srd(Kp, p.M, p.k_sm, p.D);
        const auto srd_v = head_srd(Vp, p.M, p.v_sm, p.D);
        const unsigned k0 = (k_act && kc * 8 < p.D) ? (unsigned)((kr * p.k_sm + kc * 8) * 2) : OOB_OFF, kstep = (unsigned)(KRPP * p.k_sm * 2);
        const unsigned v0 = (v_act && vc * 8 < p.D) ? (unsigned)((vr * p.v_sm + vc * 8) * 2) : OOB_OFF, vstep = (unsigned)(VRPP * p.v_sm * 2);
#pragma unroll
        for (int i = 0; i < KPASS; ++i) kreg[i] = __builtin_amdgcn_raw_buffer_load_b128(srd_k, k0 + (unsigned)i * kstep, 0, 0);
#pragma unroll
        for (int i = 0; i < VPASS; ++i) vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(srd_v, v0 + (unsigned)i * vstep, 0, 0);
    }

    // ---- park K / V: rows < sp.rows only (whole 32-key blocks up to M; the LDS image is that long), ONE barrier
    if (k_act) {
        char *kd = Kl + kr * KT::STRIDE + kc * 16;
#pragma unroll
        for (int i = 0; i < KPASS; ++i)
            if (i * KRPP + kr < sp.rows) *reinterpret_cast<u32x4 *>(kd + i * KRPP * KT::STRIDE) = kreg[i];
    }
    if (v_act) {
        char *vd = Vl + vr * VT::STRIDE + vc * 16;
#pragma unroll
        for (int i = 0; i < VPASS; ++i)
            if (i * VRPP + vr < sp.rows) *reinterpret_cast<u32x4 *>(vd + i * VRPP * VT::STRIDE) = vreg[i];
    }
    __syncthreads();

    // ---- the bias row of the lane, where the lane needs it: keys kb * 32 + 16 g + 8 hi + 0 .. 7 are 32 contiguous bytes (dword-aligned
    // buffer loads; the range check is per dword). Keys >= M of the last group read the next row's values or zeros: masked below.
    const bool biased = p.bias != nullptr && gate != 0.f;      // workgroup-uniform
    u32x4 breg[SCOPE_KB][2][2];
    if (biased) {
        const float *bbase = p.bias + b * p.b_sb + h * p.b_sh;
        const unsigned bytes = (unsigned)((((long)(p.N - 1) * p.b_sn + (long)(p.M - 1)) + 1) * 4);
        const auto srd_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(bbase), 0, bytes, 0x00020000);
        const unsigned row_off = qvalid ? (unsigned)((long)qrow * p.b_sn * 4) : OOB_OFF;
#pragma unroll
        for (int kb = 0; kb < SCOPE_KB; ++kb) {
            if (kb < nkb) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const unsigned off = row_off + (unsigned)(kb * 32 + 16 * g + 8 * hi) * 4u;
                    breg[kb][g][0] = __builtin_amdgcn_raw_buffer_load_b128(srd_b, off, 0, 0);
                    breg[kb][g][1] = __builtin_amdgcn_raw_buffer_load_b128(srd_b, off + 16u, 0, 0);
                }
            }
        }
    }

    // ---- scores of every live key block: s[kb][r] = raw score of key kb * 32 + 16 (r >> 3) + 8 hi + (r & 7) of the lane's row
    f32x16 s[SCOPE_KB];
    {
        const char *base = Kl + swap23(l31) * KT::STRIDE + hi * 16;
#pragma unroll
        for (int kb = 0; kb < SCOPE_KB; ++kb) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (kb < nkb) {
                V8 kf[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const V8 *>(base + kb * 32 * KT::STRIDE + ks * 32);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = mfma32(kf[ks], qf[ks], acc);
            }
            s[kb] = acc;
        }
    }

    // ---- the coefficient: per head from the partials, or per row from the registers
    float coeff = 0.f;
    if (biased) {
        if (head) {
            double st[4];
            parts_fold(st, pregs, sp.parts, sp.nparts, b * p.H + h, want, lane);
            if (tid == 0 && sp.stats_out && qb == 0) {
                double *so = sp.stats_out + ((long)b * p.H + h) * 4;
                so[0] = st[0]; so[1] = st[1]; so[2] = st[2]; so[3] = st[3];
            }
            coeff = stat_coefficient(c0, p.stat_kind, st, (double)p.N * (double)p.M);
        } else {
            // keys >= M were loaded as zeros: their scores are exactly 0 and leave the sum alone; the extremes and the squared
            // deviations select them out. The count is M.
            float vmax = -INFINITY, vmin = INFINITY, vsum = 0.f;
#pragma unroll
            for (int kb = 0; kb < SCOPE_KB; ++kb) {
                if (kb < nkb) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool live = key_of(kb, r, hi) < p.M;
                        const float x = s[kb][r];
                        vmax = fmaxf(vmax, live ? x : -INFINITY);
                        vmin = fminf(vmin, live ? x : INFINITY);
                        vsum += x;
                    }
                }
            }
            vmax = fmaxf(vmax, __shfl_xor(vmax, 32));
            vmin = fminf(vmin, __shfl_xor(vmin, 32));
            vsum += __shfl_xor(vsum, 32);
            const float mean = vsum / (float)p.M;
            float stat;
            if (p.stat_kind == PWW_STAT_MAX) stat = vmax;
            else if (p.stat_kind == PWW_STAT_MIN) stat = vmin;
            else if (p.stat_kind == PWW_STAT_MEAN) stat = mean;
            else if (p.stat_kind == PWW_STAT_ABSMAX) stat = fmaxf(fabsf(vmax), fabsf(vmin));
            else {      // PWW_STAT_STD: unbiased, centred (the host rejects M == 1)
                float dev = 0.f;
#pragma unroll
                for (int kb = 0; kb < SCOPE_KB; ++kb) {
                    if (kb < nkb) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float e = key_of(kb, r, hi) < p.M ? s[kb][r] - mean : 0.f;
                            dev = fmaf(e, e, dev);
                        }
                    }
                }
                dev += __shfl_xor(dev, 32);
                stat = sqrtf(dev / (float)(p.M - 1));
            }
            coeff = c0 * stat;
        }
        if (p.bias_coeff) coeff = coeff * gate;
    }

    // ---- logits x = s + c * bias (raw domain: scale > 0, so the row maximum commutes with the scaling), one-shot softmax
    const float c1 = p.scale_log2e;
    float rmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < SCOPE_KB; ++kb) {
        if (kb < nkb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float x = s[kb][r];
                if (biased) {
                    // (the element goes through a value first: __builtin_bit_cast on the element lvalue of a vector reads element 0)
                    const unsigned bits = breg[kb][r >> 3][(r >> 2) & 1][r & 3];
                    x = fmaf(__uint_as_float(bits), coeff, x);
                }
                x = key_of(kb, r, hi) < p.M ? x : -INFINITY;
                s[kb][r] = x;
                rmax = fmaxf(rmax, x);
            }
        }
    }
    rmax = xhalf_max(rmax);                      // finite: key 0 of every row is live
    const float mc = -rmax * c1;
    float psum = 0.f;
    V8 pf[SCOPE_KB][2];
#pragma unroll
    for (int kb = 0; kb < SCOPE_KB; ++kb) {
        if (kb < nkb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(s[kb][r], c1, mc));   // exp2((x - m) * scale * log2 e)
                psum += pv;
                pf[kb][r >> 3][r & 7] = (T)pv;
            }
        }
    }
    const float l_tot = psum + __shfl_xor(psum, 32);

    // ---- O^T[d][row] += V^T[d][key] * P^T[key][row]   (V^T fragments come out of the transpose read)
    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    const char *vl = Vl + vfrag_lane_off<DT>(lane);
#pragma unroll
    for (int kb = 0; kb < SCOPE_KB; ++kb) {
        if (kb < nkb) {
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const V8 vf = load_vfrag<T, DT>(vl, kb, k2, dt);
                    oacc[dt] = mfma32(vf, pf[kb][k2], oacc[dt]);
                }
            }
        }
    }
    store_o_block<T, DT>(Op + (long)(qvalid ? qrow : 0) * p.o_sn, oacc, 1.f / l_tot, p.D, hi, qvalid, p.o_wide != 0);
}

template <typename T, int KS, int DT>
static int launch_scope(const ScopeParams &sp, hipStream_t stream) {
    static_assert(ScopeGeom<KS, DT>::MAX_LDS <= 160 * 1024, "the LDS image of a workgroup must fit a compute unit");
    const size_t lds = (size_t)sp.rows * ScopeGeom<KS, DT>::ROW_BYTES;
    auto kern = scope_attn_kernel<T, KS, DT>;
    if (ScopeGeom<KS, DT>::MAX_LDS > 64 * 1024) {
        static thread_local bool attr_set[8] = {false, false, false, false, false, false, false, false};      // per device
        int dev = 0;
        if (check_hip(hipGetDevice(&dev), "hipGetDevice")) return PWW_EHIP;
        if (dev < 0 || dev >= 8 || !attr_set[dev]) {
            if (check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ScopeGeom<KS, DT>::MAX_LDS),
                          "hipFuncSetAttribute"))
                return PWW_EHIP;
            if (dev >= 0 && dev < 8) attr_set[dev] = true;
        }
    }
    const int nqb = (sp.a.N + SCOPE_NW * 32 - 1) / (SCOPE_NW * 32);
    launch_attn_kernel(kern, dim3((unsigned)nqb, (unsigned)sp.a.H, (unsigned)sp.a.B), dim3(SCOPE_NW * 64), lds, stream, sp);
    return check_hip(hipGetLastError(), "scope_attn_kernel launch");
}

template <typename T> static int dispatch_scope(const ScopeParams &sp, hipStream_t s) {
    const int D = sp.a.D;
    if (D <= 48) return launch_scope<T, 3, 2>(sp, s);
    if (D <= 64) return launch_scope<T, 4, 2>(sp, s);
    if (D <= 80) return launch_scope<T, 5, 3>(sp, s);
    if (D <= 96) return launch_scope<T, 6, 3>(sp, s);
    if (D <= 128) return launch_scope<T, 8, 4>(sp, s);
    return launch_scope<T, 10, 5>(sp, s);
}

static int scope_cross_attn(const void *q, const void *k, const void *v, void *o, const float *bias, int stat_kind, int scope, float coeff_scalar,
                            const float *gate, const pww_attn_desc_t *d, const double *parts, int nparts, double *stats_out,
                            const pww_cross_opts_t *opts, hipStream_t stream) {
    const char *me = "pww_scope_cross_attn_fwd";
    if (!q || !k || !v || !o || !d || !bias) { set_error("%s: null argument (q, k, v, o, desc, bias)", me); return PWW_EINVAL; }
    const float *coeff_dev = nullptr;
    if (opts) {
        if (opts->size < sizeof(pww_cross_opts_t)) { set_error("%s: pww_cross_opts_t.size = %u, this library needs %zu", me, opts->size, sizeof(pww_cross_opts_t)); return PWW_EINVAL; }
        coeff_dev = opts->coeff_scalar_dev;
    }
    if (int rc = check_qk(me, d)) return rc;
    if (scope != PWW_SCOPE_HEAD && scope != PWW_SCOPE_ROW) { set_error("%s: bad scope %d (PWW_SCOPE_HEAD / PWW_SCOPE_ROW)", me, scope); return PWW_EINVAL; }
    if (stat_fields_one(stat_kind) <= 0) { set_error("%s: bad statistic selector %d", me, stat_kind); return PWW_EINVAL; }
    if (stat_kind == PWW_STAT_STD && (scope == PWW_SCOPE_ROW ? d->M : (long)d->N * d->M) < 2) {
        set_error("%s: the standard deviation of a single score is undefined", me);
        return PWW_EINVAL;
    }
    if (scope == PWW_SCOPE_HEAD) {
        if (!parts) { set_error("%s: head scope needs the partials of pww_scope_head_parts", me); return PWW_EINVAL; }
        if (nparts != head_parts_count(d)) { set_error("%s: nparts = %d, this problem has %d partials per (image, head)", me, nparts, head_parts_count(d)); return PWW_EINVAL; }
    } else if (parts || nparts || stats_out) {
        set_error("%s: row scope takes no partials and writes no stats_out", me);
        return PWW_EINVAL;
    }
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(parts) || (reinterpret_cast<uintptr_t>(bias) & 3) ||
        (reinterpret_cast<uintptr_t>(stats_out) & 7) || (reinterpret_cast<uintptr_t>(gate) & 3) || (reinterpret_cast<uintptr_t>(coeff_dev) & 3)) {
        set_error("%s: q / k / v / o / partials must be 16-byte aligned, bias / gate 4-byte, stats_out 8-byte", me);
        return PWW_EINVAL;
    }
    for (int i = 0; i < 3; ++i)
        if (d->v_stride[i] % 8 || d->o_stride[i] % 4 || d->v_stride[i] < 0 || d->o_stride[i] < 0) { set_error("%s: v strides must be non-negative multiples of 8 elements (o: 4)", me); return PWW_EINVAL; }
    if (d->v_stride[2] < d->D || d->o_stride[2] < d->D) { set_error("%s: rows overlap (row stride < D)", me); return PWW_EINVAL; }
    for (int i = 0; i < 4; ++i)
        if (d->bias_stride[i] < 0) { set_error("%s: negative bias stride", me); return PWW_EINVAL; }
    if (d->bias_stride[3] != 1) { set_error("%s: the map must have unit key stride", me); return PWW_ENOTSUP; }
    if (((long)(2 * PWW_SCOPE_MAX_KEYS) * d->v_stride[2] + d->D) * 2 >= (1L << 31) || (((long)d->N + 128) * d->bias_stride[2] + 2 * PWW_SCOPE_MAX_KEYS) * 4 >= (1L << 31)) {
        set_error("%s: one (image, head) slice of v / bias must stay below 2 GiB", me);
        return PWW_ENOTSUP;
    }
    if (!(d->scale > 0.f)) { set_error("%s: scale must be positive (got %g)", me, (double)d->scale); return PWW_EINVAL; }
    if (!arch_ok()) return PWW_ENOTSUP;

    ScopeParams sp;
    memset(&sp, 0, sizeof(sp));
    AttnParams &p = sp.a;
    p.q = q; p.k = k; p.v = v; p.o = o; p.bias = bias; p.bias_coeff = gate;
    p.B = d->B; p.H = d->H; p.N = d->N; p.M = d->M; p.D = d->D;
    p.q_sb = d->q_stride[0]; p.q_sh = d->q_stride[1]; p.q_sn = d->q_stride[2];
    p.k_sb = d->k_stride[0]; p.k_sh = d->k_stride[1]; p.k_sm = d->k_stride[2];
    p.v_sb = d->v_stride[0]; p.v_sh = d->v_stride[1]; p.v_sm = d->v_stride[2];
    p.o_sb = d->o_stride[0]; p.o_sh = d->o_stride[1]; p.o_sn = d->o_stride[2];
    p.b_sb = d->bias_stride[0]; p.b_sh = d->bias_stride[1]; p.b_sn = d->bias_stride[2]; p.b_sm = 1;
    p.scale_log2e = d->scale * 1.4426950408889634f;
    p.stat_kind = stat_kind; p.coeff_scalar = coeff_scalar; p.coeff_scalar_dev = coeff_dev;
    p.o_wide = (d->o_stride[0] % 8 == 0 && d->o_stride[1] % 8 == 0 && d->o_stride[2] % 8 == 0) ? 1 : 0;
    sp.scope = scope;
    sp.parts = scope == PWW_SCOPE_HEAD ? parts : nullptr;
    sp.nparts = scope == PWW_SCOPE_HEAD ? nparts : 0;
    sp.stats_out = scope == PWW_SCOPE_HEAD ? stats_out : nullptr;
    sp.rows = (d->M + 31) & ~31;
    return d->dtype == PWW_DTYPE_F16 ? dispatch_scope<f16>(sp, stream) : dispatch_scope<bf16>(sp, stream);
}

}  // namespace pww

PWW_SCOPE_API int pww_scope_version(void) { return PWW_SCOPE_VERSION; }
PWW_SCOPE_API const char *pww_scope_last_error(void) { return pww::last_error(); }

PWW_SCOPE_API int32_t pww_scope_head_parts_count(const pww_attn_desc_t *desc) { return pww::head_parts_count(desc); }

PWW_SCOPE_API int pww_scope_head_parts(const void *q, const void *k, const float *gate, const pww_attn_desc_t *desc, int32_t stat_kind,
                                       double *partials, size_t partials_bytes, void *stream) {
    return pww::scope_head_parts(q, k, gate, desc, stat_kind, partials, partials_bytes, static_cast<hipStream_t>(stream));
}

PWW_SCOPE_API int pww_scope_cross_attn_fwd(const void *q, const void *k, const void *v, void *o, const float *bias, int32_t stat_kind, int32_t scope,
                                           float coeff_scalar, const float *gate, const pww_attn_desc_t *desc, const double *partials, int32_t nparts,
                                           double *stats_out, const pww_cross_opts_t *opts, void *stream) {
    return pww::scope_cross_attn(q, k, v, o, bias, stat_kind, scope, coeff_scalar, gate, desc, partials, nparts, stats_out, opts,
                                 static_cast<hipStream_t>(stream));
}
