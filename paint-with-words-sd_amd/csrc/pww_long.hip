// libpww_hip_long.so (include/pww_hip_long.h): the cross-attention launches of prompts encoded in 2 or 3 chunks of 77 tokens -- 128 < M <= 256 keys.
//
//   long_qk_parts_kernel   partials of the per-image score statistic over a finished Q: qk_parts_kernel of pww_cross_lean.hip with up to 8
//                          32-key blocks (the coarse form walks them, and several row blocks per wave where 256 partials per image ask for it).
//   cross_long_kernel      O = softmax((Q K^T + c[b] w) scale) V with c[b] folded from the partials at entry: cross_lean_kernel's shape --
//                          every global load of the workgroup issued before anything is waited for, every wave folds the partials itself with
//                          shuffles, one 128-row query block per workgroup -- over FOUR 64-key tiles instead of two. K / V are staged in 128-key
//                          stages: both at once for head dims <= 96 (at most 102 KB of LDS), one after the other through the same buffer above
//                          (d = 160: 84 KB per stage; the second stage's loads are in flight under the first stage's tiles). The wave's 32 bias
//                          rows are staged per 64-key tile into a wave-private piece of LDS (no barrier: LDS runs in order per wave), the next
//                          tile's rows in flight under the current tile's MFMAs; tiles past bias_cols request nothing.
//   long_probs_kernel      probs_kernel of pww_probs.hip with 8 key blocks (the attention-map recorder's launch).
//
// Traffic and arithmetic per launch against the chip's rates: DESIGN.md section 4, K8 (the one place that states them).
//
// The host helpers pww_common.h declares are this library's own (pww_side_host.h; the timing slot is below): nothing is shared with
// libpww_hip.so at link time, and only the pww_long_* entry points are visible (the unit is compiled with -fvisibility=hidden).
#include <mutex>
#define PWW_SIDE_LIB "libpww_hip_long"
#define PWW_SIDE_OWN_PROFILE
#include "pww_side_host.h"
#include "pww_attn_core.h"
#include "pww_cross_tile.h"
#include "../../include/pww_hip_long.h"

#define PWW_LONG_API extern "C" __attribute__((visibility("default")))

namespace pww {

// one timing slot (pww_long_profile_*): the event pair goes to the next launch of the arming thread
static std::mutex g_long_prof_mutex;
static hipEvent_t g_long_ev[2] = {nullptr, nullptr};
static bool g_long_used = false;
static thread_local bool g_long_armed = false;

bool profile_take(hipEvent_t *start, hipEvent_t *stop, hipStream_t stream) {
    if (!g_long_armed) return false;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return false;
    std::lock_guard<std::mutex> lock(g_long_prof_mutex);
    g_long_armed = false;
    g_long_used = true;
    *start = g_long_ev[0];
    *stop = g_long_ev[1];
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// long_qk_parts: statistic partials over a finished Q, up to 8 key blocks
// ------------------------------------------------------------------------------------------------------------------------------------
struct LongQkParams {
    const float *gate;        // [B] or null
    double *partials;         // [B][nparts][4]
    int nparts;               // partials per image
    int fields;               // bit 0 max, 1 min, 2 sum, 3 sum of squares
    int rpw;                  // COARSE: 32-row blocks a wave walks
};

constexpr int LQK_MAX_FINE = 256;      // partials per image the consumer folds from its prologue's load batch
constexpr int LQK_KB = 8;              // 32-key blocks at most

template <typename T, int KS, bool COARSE>
__global__ void __launch_bounds__(256) long_qk_parts_kernel(const void *q_, const void *k_, int q_sb, int q_sh, int q_sn, int k_sb, int k_sh, int k_sm,
                                                            int N, int M, int D, int blocks, const LongQkParams p) {
    // blocks = 32-row blocks << 4 | 32-key blocks (<= 8)
    const int nrb = blocks >> 4, nkb = blocks & 15;
    typedef typename Vec<T>::v8 V8;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z, h = blockIdx.y;
    const T *Qp = reinterpret_cast<const T *>(q_) + (long)b * q_sb + (long)h * q_sh;
    const T *Kp = reinterpret_cast<const T *>(k_) + (long)b * k_sb + (long)h * k_sh;
    const auto srd_q = head_srd(Qp, N, q_sn, D);
    const auto srd_k = head_srd(Kp, M, k_sm, D);
    const unsigned k_lane = (unsigned)((long)swap23(l31) * k_sm * 2), k_blk = (unsigned)(32 * k_sm * 2);
    const float gate = p.gate ? p.gate[b] : 1.f;
    float vmax = -INFINITY, vmin = INFINITY;
    double dsum = 0.0, dsq = 0.0;
    // one 32 x 32 block of scores into the running fields. Rows past N / keys past M were loaded as zeros (beyond the descriptors): their
    // scores are exactly 0 and leave the sums alone; the extremes take them out with a select.
    auto block = [&](const V8 (&kf)[KS], const V8 (&qf)[KS], int kb, bool rvalid) {
        int m_keys = M;
        asm volatile("" : "+v"(m_keys));              // (opaque: the key-validity masks are formed per block, not hoisted out of the row-block loop into SGPR pairs that spill)
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = mfma32(kf[ks], qf[ks], s);
        float usum = 0.f, usq = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool live = rvalid && kb * 32 + 16 * (r >> 3) + 8 * hi + (r & 7) < m_keys;
            const float x = s[r];
            vmax = fmaxf(vmax, live ? x : -INFINITY);
            vmin = fminf(vmin, live ? x : INFINITY);
            usum += x;
            usq = fmaf(x, x, usq);
        }
        dsum += (double)usum;
        dsq += (double)usq;
    };
    int rb0 = 0, kb0 = 0;
    if constexpr (COARSE) {
        // a wave walks the key blocks of `rpw` row blocks; the next K block is requested before the current one is multiplied
        rb0 = (blockIdx.x * 4 + wave) * p.rpw;
#pragma unroll 1
        for (int j = 0; j < p.rpw; ++j) {
            const int rb = rb0 + j;
            if (rb >= nrb) break;                     // (wave-uniform; the barrier below is behind the loop)
            const int qrow = rb * 32 + l31;
            V8 qf[KS], kf[2][KS];
            load_q_frags_buf<T, KS>(qf, srd_q, (unsigned)((long)qrow * q_sn * 2), hi, D);
            load_q_frags_buf<T, KS>(kf[0], srd_k, k_lane, hi, D);
#pragma unroll
            for (int kb = 0; kb < LQK_KB; ++kb) {
                if (kb + 1 < LQK_KB) load_q_frags_buf<T, KS>(kf[(kb + 1) & 1], srd_k, k_lane + (unsigned)(kb + 1) * k_blk, hi, D);      // (a block past M: beyond the descriptor)
                if (kb < nkb) block(kf[kb & 1], qf, kb, qrow < N);
            }
        }
    } else {
        const int f = blockIdx.x * 4 + wave;          // (row block, key block), key blocks fastest
        rb0 = f / nkb;
        kb0 = f - rb0 * nkb;
        if (rb0 >= nrb) return;                       // (wave-uniform; the fine form has no barrier)
        const int qrow = rb0 * 32 + l31;
        V8 qf[KS], kf[KS];
        load_q_frags_buf<T, KS>(qf, srd_q, (unsigned)((long)qrow * q_sn * 2), hi, D);
        load_q_frags_buf<T, KS>(kf, srd_k, k_lane + (unsigned)kb0 * k_blk, hi, D);
        block(kf, qf, kb0, qrow < N);
    }
    if (p.fields & 1) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off));
    }
    if (p.fields & 2) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) vmin = fminf(vmin, __shfl_xor(vmin, off));
    }
    if (p.fields & 4) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dsum += __shfl_xor(dsum, off);
    }
    if (p.fields & 8) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dsq += __shfl_xor(dsq, off);
    }
    if constexpr (COARSE) {
        __shared__ double red[4][4];
        if (lane == 0) { red[wave][0] = (double)vmax; red[wave][1] = (double)vmin; red[wave][2] = dsum; red[wave][3] = dsq; }
        __syncthreads();
        if (threadIdx.x == 0 && gate != 0.f) {
            double m = red[0][0], n = red[0][1], su = red[0][2], sq = red[0][3];
            for (int w = 1; w < 4; ++w) { m = fmax(m, red[w][0]); n = fmin(n, red[w][1]); su += red[w][2]; sq += red[w][3]; }
            double *out = p.partials + ((long)b * p.nparts + (long)h * gridDim.x + blockIdx.x) * 4;
            out[0] = (p.fields & 1) ? m : -INFINITY;
            out[1] = (p.fields & 2) ? n : INFINITY;
            out[2] = (p.fields & 4) ? su : 0.0;
            out[3] = (p.fields & 8) ? sq : 0.0;
        }
    } else if (lane == 0 && gate != 0.f) {
        double *out = p.partials + ((long)b * p.nparts + ((long)h * nrb + rb0) * nkb + kb0) * 4;
        out[0] = (p.fields & 1) ? (double)vmax : -INFINITY;
        out[1] = (p.fields & 2) ? (double)vmin : INFINITY;
        out[2] = (p.fields & 4) ? dsum : 0.0;
        out[3] = (p.fields & 8) ? dsq : 0.0;
    }
}

static bool long_shape_ok(const pww_attn_desc_t *d) {
    return d->M >= PWW_LONG_MIN_KEYS && d->M <= PWW_LONG_MAX_KEYS && d->D > 0 && d->D % 8 == 0 && d->D <= PWW_MAX_HEAD_DIM;
}

// (fine, workgroups along x per head, row blocks per wave) of the statistic launch
struct LqkPlan { bool coarse; long gx; int rpw; long nparts; };
static LqkPlan lqk_plan(const pww_attn_desc_t *d) {
    const long nrb = (d->N + 31) / 32, nkb = (d->M + 31) / 32;
    LqkPlan pl;
    pl.coarse = (long)d->H * nrb * nkb > LQK_MAX_FINE;
    pl.rpw = 1;
    if (pl.coarse) {
        while (pl.rpw < 64 && (long)d->H * ((nrb + 4 * pl.rpw - 1) / (4 * pl.rpw)) > LQK_MAX_FINE) pl.rpw *= 2;
        pl.gx = (nrb + 4 * pl.rpw - 1) / (4 * pl.rpw);
        pl.nparts = (long)d->H * pl.gx;
    } else {
        pl.gx = (nrb * nkb + 3) / 4;
        pl.nparts = (long)d->H * nrb * nkb;
    }
    return pl;
}

static int long_qk_parts_count(const pww_attn_desc_t *d) {
    if (!d || d->B <= 0 || d->H <= 0 || d->N <= 0 || !long_shape_ok(d)) return 0;
    const long n = lqk_plan(d).nparts;
    return n > 0x7fffffffL ? 0 : (int)n;
}

static int long_qk_parts(const void *q, const void *k, const float *gate, const pww_attn_desc_t *d, int stat_kind, int gated_images, double *partials,
                         size_t partials_bytes, hipStream_t stream) {
    if (!q || !k || !d || !partials) { set_error("pww_long_qk_parts: null argument"); return PWW_EINVAL; }
    if (d->B <= 0 || d->H <= 0 || d->N <= 0) { set_error("pww_long_qk_parts: empty problem"); return PWW_EINVAL; }
    if (d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) { set_error("pww_long_qk_parts: dtype %d unsupported", d->dtype); return PWW_ENOTSUP; }
    const int nparts = long_qk_parts_count(d);
    if (nparts <= 0) {
        set_error("pww_long_qk_parts: unsupported problem (B=%d H=%d N=%d M=%d D=%d; %d <= M <= %d, D a multiple of 8, <= %d)", d->B, d->H, d->N, d->M, d->D,
                  PWW_LONG_MIN_KEYS, PWW_LONG_MAX_KEYS, PWW_MAX_HEAD_DIM);
        return PWW_ENOTSUP;
    }
    const int fields = stat_fields(stat_kind);
    if (fields <= 0) { set_error("pww_long_qk_parts: bad statistic selector %d", stat_kind); return PWW_EINVAL; }
    if (!aligned16(q) || !aligned16(k) || !aligned16(partials)) { set_error("pww_long_qk_parts: q, k and partials must be 16-byte aligned"); return PWW_EINVAL; }
    for (int i = 0; i < 3; ++i) {
        if (d->q_stride[i] % 8 || d->k_stride[i] % 8) { set_error("pww_long_qk_parts: strides must be multiples of 8 elements"); return PWW_EINVAL; }
        if (d->q_stride[i] >= (1L << 31) || d->k_stride[i] >= (1L << 31) || d->q_stride[i] < 0 || d->k_stride[i] < 0) { set_error("pww_long_qk_parts: strides must be in [0, 2^31) elements"); return PWW_ENOTSUP; }
    }
    if (d->q_stride[2] < d->D || d->k_stride[2] < d->D || ((long)(d->N + 32) * d->q_stride[2] + d->D) * 2 >= (1L << 31) ||
        ((long)(PWW_LONG_MAX_KEYS + 32) * d->k_stride[2] + d->D) * 2 >= (1L << 31)) {
        set_error("pww_long_qk_parts: one head's Q / K extent must be < 2 GiB and rows must not overlap");
        return PWW_EINVAL;
    }
    if (partials_bytes < (size_t)d->B * nparts * 4 * sizeof(double)) { set_error("pww_long_qk_parts: partials buffer too small (need %zu bytes)", (size_t)d->B * nparts * 4 * sizeof(double)); return PWW_EINVAL; }
    const int n_img = (gate && gated_images > 0 && gated_images < d->B) ? gated_images : d->B;
    if (d->H > 65535 || n_img > 65535) { set_error("pww_long_qk_parts: more than 65535 heads or images"); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;
    const LqkPlan pl = lqk_plan(d);
    LongQkParams p;
    p.gate = gate; p.partials = partials; p.nparts = nparts; p.fields = fields; p.rpw = pl.rpw;
    const int nrb = (d->N + 31) / 32, nkb = (d->M + 31) / 32;
    const dim3 grid((unsigned)pl.gx, (unsigned)d->H, (unsigned)n_img);
#define PWW_LQK_ARGS q, k, (int)d->q_stride[0], (int)d->q_stride[1], (int)d->q_stride[2], (int)d->k_stride[0], (int)d->k_stride[1], (int)d->k_stride[2], \
                     (int)d->N, (int)d->M, (int)d->D, (nrb << 4) | nkb, p
#define PWW_LQK1(T, KSV)                                                                                               \
    do {                                                                                                                \
        if (pl.coarse) launch_timed(long_qk_parts_kernel<T, KSV, true>, grid, dim3(256), 0, stream, PWW_LQK_ARGS);      \
        else launch_timed(long_qk_parts_kernel<T, KSV, false>, grid, dim3(256), 0, stream, PWW_LQK_ARGS);               \
    } while (0)
#define PWW_LQK(T)                                      \
    do {                                                \
        const int ks = (d->D + 15) / 16;                \
        if (ks <= 3) PWW_LQK1(T, 3);                    \
        else if (ks == 4) PWW_LQK1(T, 4);               \
        else if (ks == 5) PWW_LQK1(T, 5);               \
        else if (ks == 6) PWW_LQK1(T, 6);               \
        else if (ks <= 8) PWW_LQK1(T, 8);               \
        else PWW_LQK1(T, 10);                           \
    } while (0)
    if (d->dtype == PWW_DTYPE_F16) PWW_LQK(f16); else PWW_LQK(bf16);
#undef PWW_LQK
#undef PWW_LQK1
#undef PWW_LQK_ARGS
    return check_hip(hipGetLastError(), "long_qk_parts_kernel launch");
}

// ------------------------------------------------------------------------------------------------------------------------------------
// cross_long: pass-2-only cross-attention over up to four 64-key tiles, one 128-row query block per workgroup
// ------------------------------------------------------------------------------------------------------------------------------------
struct LongParams {
    AttnParams a;             // a.bias_coeff = the row gate [B] (or null)
    const double *parts;      // [B][nparts][4] or null (stat_kind == NONE)
    int nparts;
    double *stats_out;        // optional [B][4]
};

constexpr int LONG_NW = 4;                 // waves per workgroup: 128 query rows
constexpr int LONG_STAGE = 2 * KVBLK;      // key rows of a K / V stage
constexpr int LONG_TILE_STRIDE = 64;       // floats per row of the bias tile: the columns of one 64-key tile
constexpr int LONG_TILE_LOADS = 8;         // 16-byte pieces per lane of a wave's 32 bias rows x 64 columns
constexpr int LONG_TILE_BYTES = LONG_NW * 32 * LONG_TILE_STRIDE * 4;

template <int KS, int DT> struct LongGeom {
    static constexpr bool RES = DT <= 3;                       // both stages resident in LDS (d <= 96)
    static constexpr int ROWS = RES ? 2 * LONG_STAGE : LONG_STAGE;    // key rows the LDS image has room for
    static constexpr int NST = RES ? 1 : 2;                    // stages walked through it
    static constexpr int K_BYTES = ROWS * KTile<KS>::STRIDE, V_BYTES = ROWS * VTile<DT>::STRIDE;
    static constexpr size_t LDS = (size_t)K_BYTES + V_BYTES + LONG_TILE_BYTES;
};

template <typename T, int KS, int DT>
__global__ void __launch_bounds__(LONG_NW * 64, 1) cross_long_kernel(const LongParams lp) {
    typedef typename Vec<T>::v8 V8;
    typedef KTile<KS> KT;
    typedef VTile<DT> VT;
    typedef LongGeom<KS, DT> G;
    constexpr bool RSM = KS * 16 < DT * 32;      // padding channels in the V tile: channel D is a column of ones, the PV MFMAs deliver the row sums
    constexpr int NT = LONG_NW * 64;
    constexpr int KRPP = NT / KT::CHK, VRPP = NT / VT::CHK;                   // key rows a pass of the workgroup covers
    constexpr int KPASS = (G::ROWS + KRPP - 1) / KRPP, VPASS = (G::ROWS + VRPP - 1) / VRPP;
    constexpr int TPS = G::ROWS / KVBLK;         // 64-key tiles per stage
    const AttnParams &p = lp.a;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *Kl = smem, *Vl = smem + G::K_BYTES, *tile = smem + G::K_BYTES + G::V_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, l31 = lane & 31;
    const int qb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;

    // ---- every global load of the workgroup's first stage, before anything is waited for: gate, partials, Q fragments, K / V chunks, bias rows
    const float gate = p.bias_coeff ? p.bias_coeff[b] : 1.f;
    const float c0 = coeff_scalar_of(p);
    const bool need_stat = p.stat_kind != PWW_STAT_NONE;
    const PartsWant want(p.stat_kind, lp.stats_out != nullptr);
    PartsRegs pr;
    parts_request(pr, lp.parts, lp.nparts, b, need_stat, want, lane);
    const T *Qp = reinterpret_cast<const T *>(p.q) + b * p.q_sb + h * p.q_sh;
    const T *Kp = reinterpret_cast<const T *>(p.k) + b * p.k_sb + h * p.k_sh;
    const T *Vp = reinterpret_cast<const T *>(p.v) + b * p.v_sb + h * p.v_sh;
    T *Op = reinterpret_cast<T *>(p.o) + b * p.o_sb + h * p.o_sh;
    const int qrow = (qb * LONG_NW + wave) * 32 + l31;
    const bool qvalid = qrow < p.N;
    V8 qf[KS];
    const auto srd_q = head_srd(Qp, p.N, p.q_sn, p.D);
    load_q_frags_buf<T, KS>(qf, srd_q, (unsigned)((long)qrow * p.q_sn * 2), hi, p.D);      // (rows past N: beyond the descriptor)

    // K / V: thread -> (row kr of a pass, 16-byte column kc); pass i = rows i * KRPP .. of the stage. Rows past M, the head-dim padding and
    // idle threads are out of range of the descriptor: zeros, no memory traffic, no compare per chunk.
    u32x4 kreg[KPASS], vreg[VPASS];
    const int kr = tid / KT::CHK, kc = tid - kr * KT::CHK;
    const int vr = tid / VT::CHK, vc = tid - vr * VT::CHK;
    const bool k_act = kr < KRPP, v_act = vr < VRPP;
    const auto srd_k = head_srd(Kp, p.M, p.k_sm, p.D);
    const auto srd_v = head_srd(Vp, p.M, p.v_sm, p.D);
    const unsigned k0 = (k_act && kc * 8 < p.D) ? (unsigned)((kr * p.k_sm + kc * 8) * 2) : OOB_OFF, kstep = (unsigned)(KRPP * p.k_sm * 2);
    const unsigned v0 = (v_act && vc * 8 < p.D) ? (unsigned)((vr * p.v_sm + vc * 8) * 2) : OOB_OFF, vstep = (unsigned)(VRPP * p.v_sm * 2);
    auto stage_request = [&](int st) {
        const unsigned ks0 = (unsigned)(st * G::ROWS * p.k_sm * 2), vs0 = (unsigned)(st * G::ROWS * p.v_sm * 2);
#pragma unroll
        for (int i = 0; i < KPASS; ++i) kreg[i] = __builtin_amdgcn_raw_buffer_load_b128(srd_k, k0 + ks0 + (unsigned)i * kstep, 0, 0);
#pragma unroll
        for (int i = 0; i < VPASS; ++i) vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(srd_v, v0 + vs0 + (unsigned)i * vstep, 0, 0);
    };
    stage_request(0);

    // bias rows of THIS WAVE's 32 query rows, the 64 columns of one key tile at a time: lane -> (row rowl0 of a pass of 4 rows, 16-byte column pc)
    const int pc = lane & 15, rowl0 = lane >> 4;
    const unsigned bbytes = (unsigned)((((long)(p.N - 1) * p.b_sn + (long)(p.M - 1) * p.b_sm) + 1) * 4);
    const float *bbase = p.bias + b * p.b_sb + h * p.b_sh;
    const auto srd_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(bbase), 0, bbytes, 0x00020000);
    // (rows past N lie beyond the descriptor for a dense map; columns past bias_cols are never requested, stored or read)
    const unsigned t_row = (unsigned)((((long)(qb * LONG_NW + wave) * 32 + rowl0) * p.b_sn + pc * 4) * 4), tstep = (unsigned)(4 * p.b_sn * 4);
    u32x4 treg[LONG_TILE_LOADS];
    auto tile_request = [&](int gt) {
        const unsigned t0 = gt * KVBLK + pc * 4 < p.bias_cols ? t_row + (unsigned)(gt * KVBLK * 4) : OOB_OFF;
#pragma unroll
        for (int i = 0; i < LONG_TILE_LOADS; ++i) treg[i] = __builtin_amdgcn_raw_buffer_load_b128(srd_b, t0 + (unsigned)i * tstep, 0, 0);
    };
    auto tile_park = [&](int gt) {
        if (gt * KVBLK + pc * 4 < p.bias_cols) {
#pragma unroll
            for (int i = 0; i < LONG_TILE_LOADS; ++i) {
                const int row = wave * 32 + rowl0 + i * 4;
                *reinterpret_cast<u32x4 *>(tile + (long)row * LONG_TILE_STRIDE * 4 + ((pc ^ tile_swz(row, LONG_TILE_STRIDE / 4)) << 4)) = treg[i];
            }
        }
    };
    tile_request(0);

    // ---- fold the image's partials: EVERY WAVE folds all of them itself (shuffles only). The same order in every wave of every workgroup.
    float coeff = 0.f;
    const bool biased = gate != 0.f;      // workgroup-uniform
    if (biased) {
        coeff = c0;
        if (need_stat) {
            double st[4];
            parts_fold(st, pr, lp.parts, lp.nparts, b, want, lane);
            if (tid == 0 && lp.stats_out && h == 0 && qb == 0) {
                double *so = lp.stats_out + (long)b * 4;
                so[0] = st[0]; so[1] = st[1]; so[2] = st[2]; so[3] = st[3];
            }
            coeff = stat_coefficient(c0, p.stat_kind, st, p.stat_count);
        }
        if (p.bias_coeff) coeff = coeff * gate;
    }
    BiasRef bias;
    bias_ref_tile(bias, tile, wave * 32 + l31, LONG_TILE_STRIDE, 0, hi);
    // a gated-out image (an unconditional row of a CFG-folded batch) reads no column of the tile: its logits are the plain scores
    const int cols = biased ? p.bias_cols : 0;

    const float c1 = p.scale_log2e;
    f32x16 oacc[DT];
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (p.M + KVBLK - 1) / KVBLK;      // 3 or 4
    const T one = (T)1.0f;
    unsigned short one_bits;
    __builtin_memcpy(&one_bits, &one, 2);
    const bool v_one = RSM && vc * 8 == p.D;           // first padding chunk: channel D = 1.0 (the softmax denominator's column)

#pragma unroll
    for (int st = 0; st < G::NST; ++st) {
        // ---- park the stage's K / V (whole 32-key blocks up to M: rows past M arrived as zeros) and, for the first stage, the wave's bias rows
        if (st > 0) __syncthreads();                   // every wave is done with the previous stage's K / V
        const int rows = min(G::ROWS, ((p.M + 31) & ~31) - st * G::ROWS);
        if (k_act) {
            char *kd = Kl + kr * KT::STRIDE + kc * 16;
#pragma unroll
            for (int i = 0; i < KPASS; ++i)
                if (i * KRPP < rows && ((i + 1) * KRPP <= G::ROWS || i * KRPP + kr < G::ROWS))      // (first test uniform; the second a constant except in the last pass)
                    *reinterpret_cast<u32x4 *>(kd + i * KRPP * KT::STRIDE) = kreg[i];
        }
        if (v_act) {
            char *vd = Vl + vr * VT::STRIDE + vc * 16;
#pragma unroll
            for (int i = 0; i < VPASS; ++i)
                if (i * VRPP < rows && ((i + 1) * VRPP <= G::ROWS || i * VRPP + vr < G::ROWS))
                    *reinterpret_cast<u32x4 *>(vd + i * VRPP * VT::STRIDE) = v_one ? u32x4{(unsigned)one_bits, 0u, 0u, 0u} : vreg[i];
        }
        if (st == 0) tile_park(0);
        if (st + 1 < G::NST) stage_request(st + 1);    // in flight under this stage's tiles
        __syncthreads();

        // ---- scores -> (bias) -> softmax -> PV, tile by tile. Tile 0 is all live, sets the row's reference and starts O^T from a zero constant
        // (STEP 1); the later tiles keep that reference unless a score exceeds it by 2^8 (STEP 2); tiles 2 and 3 may be ragged or absent.
        // A tile is handed to attn_tile with the key axis shifted to its own start: key0 = 0, M and the column bound less the tile's offset.
#pragma unroll
        for (int tt = 0; tt < TPS; ++tt) {
            const int gt = st * TPS + tt;
            if (gt < ntiles) {                         // (workgroup-uniform)
                if (gt + 1 < ntiles) tile_request(gt + 1);
                bias.lds_cols = cols - gt * KVBLK;
                const char *Kt = Kl + tt * KT::BYTES, *Vt = Vl + tt * VT::BYTES;
                if (gt == 0) attn_tile<T, KS, DT, 2, false, RSM, 1>(oacc, m_run, l_run, qf, Kt, Vt, 0, p.M, l31, hi, bias, coeff, c1);
                else if (gt == 1) attn_tile<T, KS, DT, 2, false, RSM, 2>(oacc, m_run, l_run, qf, Kt, Vt, 0, p.M - KVBLK, l31, hi, bias, coeff, c1);
                else attn_tile<T, KS, DT, 2, true, RSM, 2>(oacc, m_run, l_run, qf, Kt, Vt, 0, p.M - gt * KVBLK, l31, hi, bias, coeff, c1);
                // the wave's own rows of the tile: its reads of the tile just computed are behind it in program order (LDS runs in order per wave)
                if (gt + 1 < ntiles) tile_park(gt + 1);
            }
        }
    }
    float l_tot;
    if (RSM) {      // row D of O^T: tile D / 32, register (D % 32) / 2, held by the hi == 0 half
        const int rl = p.D & 31, tl = p.D >> 5;
        float lv = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const float c = rl == 0 ? oacc[dt][0] : rl == 8 ? oacc[dt][4] : rl == 16 ? oacc[dt][8] : oacc[dt][12];
            lv = dt == tl ? c : lv;
        }
        const float other = __shfl_xor(lv, 32);
        l_tot = hi ? other : lv;
    } else {
        l_tot = l_run + __shfl_xor(l_run, 32);
    }
    const float inv = 1.f / l_tot;
    store_o_block<T, DT>(Op + (long)(qvalid ? qrow : 0) * p.o_sn, oacc, inv, p.D, hi, qvalid, p.o_wide != 0);
}

template <typename T, int KS, int DT>
static int launch_long(const LongParams &lp, hipStream_t stream) {
    constexpr size_t lds = LongGeom<KS, DT>::LDS;
    static_assert(lds <= 160 * 1024, "the LDS image of a workgroup must fit a compute unit");
    auto kern = cross_long_kernel<T, KS, DT>;
    static thread_local bool attr_set[8] = {false, false, false, false, false, false, false, false};      // per device
    int dev = 0;
    if (check_hip(hipGetDevice(&dev), "hipGetDevice")) return PWW_EHIP;
    if (dev < 0 || dev >= 8 || !attr_set[dev]) {
        if (check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute"))
            return PWW_EHIP;
        if (dev >= 0 && dev < 8) attr_set[dev] = true;
    }
    const int nqb = (lp.a.N + LONG_NW * 32 - 1) / (LONG_NW * 32);
    launch_attn_kernel(kern, dim3((unsigned)nqb, (unsigned)lp.a.H, (unsigned)lp.a.B), dim3(LONG_NW * 64), lds, stream, lp);
    return check_hip(hipGetLastError(), "cross_long_kernel launch");
}

template <typename T> static int dispatch_long(const LongParams &lp, hipStream_t s) {
    const int D = lp.a.D;
    if (D <= 48) return launch_long<T, 3, 2>(lp, s);
    if (D <= 64) return launch_long<T, 4, 2>(lp, s);
    if (D <= 80) return launch_long<T, 5, 3>(lp, s);
    if (D <= 96) return launch_long<T, 6, 3>(lp, s);
    if (D <= 128) return launch_long<T, 8, 4>(lp, s);
    return launch_long<T, 10, 5>(lp, s);
}

static int long_cross_attn(const void *q, const void *k, const void *v, void *o, const float *bias, int stat_kind, float coeff_scalar, const float *gate,
                           const pww_attn_desc_t *d, const double *parts, int nparts, double *stats_out, const pww_cross_opts_t *opts, hipStream_t stream) {
    const char *me = "pww_long_cross_attn_fwd_parts";
    if (!q || !k || !v || !o || !d || !bias) { set_error("%s: null argument (q, k, v, o, desc, bias)", me); return PWW_EINVAL; }
    const float *coeff_dev = nullptr;
    int bias_cols = 0;
    if (opts) {
        if (opts->size < sizeof(pww_cross_opts_t)) { set_error("%s: pww_cross_opts_t.size = %u, this library needs %zu", me, opts->size, sizeof(pww_cross_opts_t)); return PWW_EINVAL; }
        if (opts->bias_compact || opts->col_idx) { set_error("%s: the compact form of the map is not taken", me); return PWW_ENOTSUP; }
        if (opts->bias_cols < 0) { set_error("%s: negative bias_cols", me); return PWW_EINVAL; }
        coeff_dev = opts->coeff_scalar_dev;
        bias_cols = opts->bias_cols;
    }
    if (d->B <= 0 || d->H <= 0 || d->N <= 0 || d->M <= 0 || d->D <= 0) { set_error("%s: non-positive dimension (B=%d H=%d N=%d M=%d D=%d)", me, d->B, d->H, d->N, d->M, d->D); return PWW_EINVAL; }
    if (!long_shape_ok(d)) {
        set_error("%s: unsupported problem (M=%d D=%d; %d <= M <= %d, D a multiple of 8, <= %d)", me, d->M, d->D, PWW_LONG_MIN_KEYS, PWW_LONG_MAX_KEYS, PWW_MAX_HEAD_DIM);
        return PWW_ENOTSUP;
    }
    if (d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) { set_error("%s: dtype %d unsupported", me, d->dtype); return PWW_ENOTSUP; }
    if (stat_kind < PWW_STAT_NONE || stat_kind > PWW_STAT_ABSMAX) { set_error("%s: bad statistic selector %d", me, stat_kind); return PWW_EINVAL; }
    if (stat_kind != PWW_STAT_NONE && (!parts || nparts <= 0)) { set_error("%s: a statistic needs its partials", me); return PWW_EINVAL; }
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(parts) || (reinterpret_cast<uintptr_t>(bias) & 3) ||
        (reinterpret_cast<uintptr_t>(stats_out) & 7) || (reinterpret_cast<uintptr_t>(gate) & 3) || (reinterpret_cast<uintptr_t>(coeff_dev) & 3)) {
        set_error("%s: q / k / v / o / partials must be 16-byte aligned, bias / gate 4-byte, stats_out 8-byte", me);
        return PWW_EINVAL;
    }
    for (int i = 0; i < 3; ++i) {
        if (d->q_stride[i] % 8 || d->k_stride[i] % 8 || d->v_stride[i] % 8 || d->o_stride[i] % 4 || d->q_stride[i] < 0 || d->k_stride[i] < 0 ||
            d->v_stride[i] < 0 || d->o_stride[i] < 0) {
            set_error("%s: strides must be non-negative multiples of 8 elements (o: 4)", me);
            return PWW_EINVAL;
        }
    }
    if (d->q_stride[2] < d->D || d->k_stride[2] < d->D || d->v_stride[2] < d->D || d->o_stride[2] < d->D) { set_error("%s: rows overlap (row stride < D)", me); return PWW_EINVAL; }
    for (int i = 0; i < 4; ++i)
        if (d->bias_stride[i] < 0) { set_error("%s: negative bias stride", me); return PWW_EINVAL; }
    if (d->bias_stride[3] != 1) { set_error("%s: the map must have unit key stride", me); return PWW_ENOTSUP; }
    // (the kernel forms 32-bit byte offsets of rows just past N / M before the descriptors cut them off)
    if (((long)(d->N + 128) * d->q_stride[2] + d->D) * 2 >= (1L << 31) || ((long)(2 * PWW_LONG_MAX_KEYS) * d->k_stride[2] + d->D) * 2 >= (1L << 31) ||
        ((long)(2 * PWW_LONG_MAX_KEYS) * d->v_stride[2] + d->D) * 2 >= (1L << 31) || ((long)(d->N + 128) * d->bias_stride[2] + 2 * PWW_LONG_MAX_KEYS) * 4 >= (1L << 31)) {
        set_error("%s: one (image, head) slice of q / k / v / bias must stay below 2 GiB", me);
        return PWW_ENOTSUP;
    }
    if (!(d->scale > 0.f)) { set_error("%s: scale must be positive (got %g)", me, (double)d->scale); return PWW_EINVAL; }
    if (d->H > 65535 || d->B > 65535) { set_error("%s: more than 65535 heads or images", me); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;

    const int m16 = (d->M + 15) & ~15;
    bias_cols = bias_cols > 0 ? ((bias_cols + 15) & ~15) : m16;
    if (bias_cols > m16) bias_cols = m16;
    LongParams lp;
    memset(&lp, 0, sizeof(lp));
    AttnParams &p = lp.a;
    p.q = q; p.k = k; p.v = v; p.o = o; p.bias = bias; p.bias_coeff = gate;
    p.B = d->B; p.H = d->H; p.N = d->N; p.M = d->M; p.D = d->D;
    p.q_sb = d->q_stride[0]; p.q_sh = d->q_stride[1]; p.q_sn = d->q_stride[2];
    p.k_sb = d->k_stride[0]; p.k_sh = d->k_stride[1]; p.k_sm = d->k_stride[2];
    p.v_sb = d->v_stride[0]; p.v_sh = d->v_stride[1]; p.v_sm = d->v_stride[2];
    p.o_sb = d->o_stride[0]; p.o_sh = d->o_stride[1]; p.o_sn = d->o_stride[2];
    p.b_sb = d->bias_stride[0]; p.b_sh = d->bias_stride[1]; p.b_sn = d->bias_stride[2]; p.b_sm = 1;
    p.scale_log2e = d->scale * 1.4426950408889634f;
    p.stat_kind = stat_kind; p.stat_count = (double)d->H * d->N * d->M; p.coeff_scalar = coeff_scalar; p.coeff_scalar_dev = coeff_dev;
    p.bias_cols = bias_cols;
    p.o_wide = (d->o_stride[0] % 8 == 0 && d->o_stride[1] % 8 == 0 && d->o_stride[2] % 8 == 0) ? 1 : 0;
    lp.parts = stat_kind != PWW_STAT_NONE ? parts : nullptr;
    lp.nparts = stat_kind != PWW_STAT_NONE ? nparts : 0;
    lp.stats_out = stat_kind != PWW_STAT_NONE ? stats_out : nullptr;
    return d->dtype == PWW_DTYPE_F16 ? dispatch_long<f16>(lp, stream) : dispatch_long<bf16>(lp, stream);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// long_probs: head-averaged softmax probabilities over up to 8 key blocks
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int LPROBS_NW = 4;           // waves per workgroup: the heads are dealt round-robin to them
constexpr int LPROBS_KB = 8;           // 32-key blocks at most (M <= 256)
constexpr int LPROBS_STRIDE = 260;     // floats per LDS tile row: 256 keys + 4 (a lane's 16-byte pieces of consecutive rows fall into different banks)

struct LongProbsParams {
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

// One workgroup of four waves owns a 32-row query block of one image; wave w walks the heads w, w + 4, ... and sums their normalised
// probabilities in registers, heads in ascending order. The four sums meet in ONE LDS tile in a fixed order -- wave 0 stores, waves 1, 2, 3
// add to it in turn -- and the block is written with the keys on the lane axis. One owner per output element, no atomics.
template <typename T>
__global__ void __launch_bounds__(LPROBS_NW * 64) long_probs_kernel(const LongProbsParams p) {
    typedef typename Vec<T>::v8 V8;
    __shared__ __attribute__((aligned(16))) float tile[32 * LPROBS_STRIDE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, l31 = lane & 31;
    const int rb = blockIdx.x, b = blockIdx.y;
    const int qrow = rb * 32 + l31;

    float coeff = 0.f;
    if (p.bias) {
        const float gate = p.gate ? p.gate[b] : 1.f;
        if (gate != 0.f) {                            // (a gated-out image's statistics may never have been written)
            coeff = p.coeff_scalar_dev ? *p.coeff_scalar_dev : p.coeff_scalar;
            if (p.stat_kind != PWW_STAT_NONE) coeff = stat_coefficient(coeff, p.stat_kind, p.stats + (long)b * 4, p.stat_count);
            if (p.gate) coeff = coeff * gate;
        }
    }

    float acc[LPROBS_KB][16];
#pragma unroll
    for (int kb = 0; kb < LPROBS_KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kb][r] = 0.f;

    const unsigned q_off = (unsigned)((long)qrow * p.q_sn * 2);
    const unsigned k_lane = (unsigned)((long)swap23(l31) * p.k_sm * 2), k_blk = (unsigned)(32 * p.k_sm * 2);
    const unsigned b_row = (unsigned)((long)qrow * p.b_sn * 4);
    const float c2 = p.scale * 1.44269504088896340736f;      // the exponentials run as exp2
    const int nks = (p.D + 15) >> 4;                  // 16-wide contraction steps, a RUN-TIME bound
    const unsigned d_lane = (unsigned)hi * 16u;
    const bool d_tail = (p.D & 8) != 0;               // the last step's upper half lies past D

    for (int h = wave; h < p.H; h += LPROBS_NW) {     // (wave-uniform trip count)
        const T *Qp = reinterpret_cast<const T *>(p.q) + b * p.q_sb + h * p.q_sh;
        const T *Kp = reinterpret_cast<const T *>(p.k) + b * p.k_sb + h * p.k_sh;
        const auto srd_q = head_srd(Qp, p.N, p.q_sn, p.D);
        const auto srd_k = head_srd(Kp, p.M, p.k_sm, p.D);
        f32x16 s[LPROBS_KB];
#pragma unroll
        for (int kb = 0; kb < LPROBS_KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
        // rows past N, key blocks past M and the half step past D lie beyond the descriptors (or get an out-of-range offset): zeros
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
            const bool live = !(d_tail && hi && ks == nks - 1);
            const unsigned d_off = (unsigned)ks * 32u + d_lane;
            u32x4 f[1 + LPROBS_KB];
            f[0] = __builtin_amdgcn_raw_buffer_load_b128(srd_q, live ? q_off + d_off : OOB_OFF, 0, 0);
#pragma unroll
            for (int kb = 0; kb < LPROBS_KB; ++kb)
                f[1 + kb] = __builtin_amdgcn_raw_buffer_load_b128(srd_k, live ? k_lane + (unsigned)kb * k_blk + d_off : OOB_OFF, 0, 0);
#pragma unroll
            for (int kb = 0; kb < LPROBS_KB; ++kb) s[kb] = mfma32(__builtin_bit_cast(V8, f[1 + kb]), __builtin_bit_cast(V8, f[0]), s[kb]);
        }
        if (p.bias) {
            const float *bbase = p.bias + b * p.b_sb + h * p.b_sh;
            const unsigned bytes = (unsigned)(((long)(p.N - 1) * p.b_sn + (long)(p.M - 1) * p.b_sm + 1) * 4);
            const auto srd_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(bbase), 0, bytes, 0x00020000);
            unsigned kstep = (unsigned)(p.b_sm * 4);
            asm volatile("" : "+v"(kstep));           // (opaque: the products key * stride are formed where they are used)
#pragma unroll
            for (int kb = 0; kb < LPROBS_KB; ++kb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned off = b_row + (unsigned)(key_of(0, r, hi) + kb * 32) * kstep;
                    s[kb][r] = fmaf(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_b, off, 0, 0)), coeff, s[kb][r]);
                }
            }
        }
        // keys past M leave the softmax (that includes whole key blocks past M: exp2(-inf) = 0)
        float mx = -INFINITY;
        int m_keys = p.M;
        asm volatile("" : "+v"(m_keys));              // (opaque: the 128 key-validity masks are formed per head, not hoisted into SGPR pairs that spill)
#pragma unroll
        for (int kb = 0; kb < LPROBS_KB; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t = key_of(0, r, hi) + kb * 32 < m_keys ? s[kb][r] * c2 : -INFINITY;
                s[kb][r] = t;
                mx = fmaxf(mx, t);
            }
        }
        mx = xhalf_max(mx);                           // finite: key 0 of the row is live
        float l = 0.f;
#pragma unroll
        for (int kb = 0; kb < LPROBS_KB; ++kb) {
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
        for (int kb = 0; kb < LPROBS_KB; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kb][r] = fmaf(s[kb][r], inv, acc[kb][r]);
        }
    }

    // ---- the four waves' sums meet in LDS, fixed order ((w0 + w1) + w2) + w3: every wave addresses the tile alike (lane -> row l31, 8
    // consecutive keys per piece)
    float *mine = tile + l31 * LPROBS_STRIDE + 8 * hi;
#pragma unroll 1
    for (int w = 0; w < LPROBS_NW; ++w) {
        if (wave == w) {
#pragma unroll
            for (int kb = 0; kb < LPROBS_KB; ++kb) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 *dst = reinterpret_cast<f32x4 *>(mine + kb * 32 + 16 * (g >> 1) + 4 * (g & 1));
                    f32x4 v = f32x4{acc[kb][g * 4], acc[kb][g * 4 + 1], acc[kb][g * 4 + 2], acc[kb][g * 4 + 3]};
                    if (w > 0) { const f32x4 old = *dst; v = f32x4{old[0] + v[0], old[1] + v[1], old[2] + v[2], old[3] + v[3]}; }
                    *dst = v;
                }
            }
        }
        __syncthreads();
    }

    // ---- store: thread -> (row t >> 6 of a pass of 4 rows, keys 4 (t & 63) .. + 3)
    const int c4 = threadIdx.x & 63, key0 = c4 * 4;
    const float hf = (float)p.H;
    if (key0 < p.M) {
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const int r = (threadIdx.x >> 6) + 4 * i, n = rb * 32 + r;
            if (n < p.N) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(tile + r * LPROBS_STRIDE + key0);
                float *dst = p.out + b * p.o_sb + n * p.o_sn + key0;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = p.weight * (a[j] / hf);
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

static int lprobs_fail(int rc, const char *msg) { set_error("pww_long_cross_attn_probs: %s", msg); return rc; }

static int long_probs(const void *q, const void *k, const float *bias, const double *stats, int stat_kind, double stat_count, float coeff_scalar,
                      const float *gate, const pww_attn_desc_t *d, const pww_cross_opts_t *opts, float *out, const pww_probs_desc_t *pd, hipStream_t st) {
    if (!q || !k || !d || !out || !pd) return lprobs_fail(PWW_EINVAL, "null argument (q, k, desc, out, pdesc)");
    if (pd->size < sizeof(pww_probs_desc_t)) {
        set_error("pww_long_cross_attn_probs: pww_probs_desc_t.size = %u, this library needs %zu", pd->size, sizeof(pww_probs_desc_t));
        return PWW_EINVAL;
    }
    const float *coeff_dev = nullptr;
    if (opts) {
        if (opts->size < 16) { set_error("pww_long_cross_attn_probs: pww_cross_opts_t.size = %u is not a known layout", opts->size); return PWW_EINVAL; }
        coeff_dev = opts->coeff_scalar_dev;
    }
    if (d->B <= 0 || d->H <= 0 || d->N <= 0 || d->M <= 0 || d->D <= 0) return lprobs_fail(PWW_EINVAL, "empty problem");
    if (stat_kind < PWW_STAT_NONE || stat_kind > PWW_STAT_ABSMAX) return lprobs_fail(PWW_EINVAL, "bad statistic selector");
    if (stat_kind != PWW_STAT_NONE && !stats) return lprobs_fail(PWW_EINVAL, "null stats with a statistic selected");
    if (pd->images < 0 || pd->images > d->B) return lprobs_fail(PWW_EINVAL, "images must be 0 (all) or at most B");
    if (pd->accumulate != 0 && pd->accumulate != 1) return lprobs_fail(PWW_EINVAL, "accumulate must be 0 or 1");
    if (d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) return lprobs_fail(PWW_ENOTSUP, "dtype unsupported");
    if (!long_shape_ok(d)) {
        set_error("pww_long_cross_attn_probs: unsupported problem (M=%d D=%d; %d <= M <= %d, D a multiple of 8, <= %d)", d->M, d->D, PWW_LONG_MIN_KEYS,
                  PWW_LONG_MAX_KEYS, PWW_MAX_HEAD_DIM);
        return PWW_ENOTSUP;
    }
    if (!aligned16(q) || !aligned16(k) || !aligned16(out) || (reinterpret_cast<uintptr_t>(bias) & 3) || (reinterpret_cast<uintptr_t>(stats) & 7) ||
        (reinterpret_cast<uintptr_t>(gate) & 3) || (reinterpret_cast<uintptr_t>(coeff_dev) & 3))
        return lprobs_fail(PWW_EINVAL, "q, k and out must be 16-byte aligned, bias / gate 4-byte, stats 8-byte");
    for (int i = 0; i < 3; ++i)
        if (d->q_stride[i] % 8 || d->k_stride[i] % 8 || d->q_stride[i] < 0 || d->k_stride[i] < 0) return lprobs_fail(PWW_EINVAL, "q / k strides must be non-negative multiples of 8 elements");
    if (d->q_stride[2] < d->D || d->k_stride[2] < d->D) return lprobs_fail(PWW_EINVAL, "q / k rows overlap (row stride < D)");
    if (pd->out_stride[1] < d->M || pd->out_stride[1] % 4 || pd->out_stride[0] % 4 || pd->out_stride[0] < 0)
        return lprobs_fail(PWW_EINVAL, "out row stride must be >= M and, like the image stride, a multiple of 4 floats");
    if (bias)
        for (int i = 0; i < 4; ++i)
            if (d->bias_stride[i] < 0) return lprobs_fail(PWW_EINVAL, "negative bias stride");
    if (((long)(d->N + 32) * d->q_stride[2] + d->D) * 2 >= (1L << 31) || ((long)(32 * LPROBS_KB + 32) * d->k_stride[2] + d->D) * 2 >= (1L << 31) ||
        (bias && ((long)(d->N + 32) * d->bias_stride[2] + (long)(32 * LPROBS_KB + 32) * d->bias_stride[3] + 1) * 4 >= (1L << 31)))
        return lprobs_fail(PWW_ENOTSUP, "one (image, head) slice of q / k / bias must stay below 2 GiB");
    const int images = pd->images ? pd->images : d->B;
    const long nrb = ((long)d->N + 31) / 32;
    if (images > 65535) return lprobs_fail(PWW_ENOTSUP, "more than 65535 images");
    if (!arch_ok()) return PWW_ENOTSUP;

    LongProbsParams p;
    p.q = q; p.k = k; p.bias = bias; p.stats = stats; p.gate = gate; p.coeff_scalar_dev = coeff_dev; p.out = out;
    p.H = d->H; p.N = d->N; p.M = d->M; p.D = d->D;
    p.q_sb = d->q_stride[0]; p.q_sh = d->q_stride[1]; p.q_sn = d->q_stride[2];
    p.k_sb = d->k_stride[0]; p.k_sh = d->k_stride[1]; p.k_sm = d->k_stride[2];
    p.b_sb = bias ? d->bias_stride[0] : 0; p.b_sh = bias ? d->bias_stride[1] : 0; p.b_sn = bias ? d->bias_stride[2] : 0; p.b_sm = bias ? d->bias_stride[3] : 0;
    p.o_sb = pd->out_stride[0]; p.o_sn = pd->out_stride[1];
    p.scale = d->scale; p.coeff_scalar = coeff_scalar; p.weight = pd->weight;
    p.stat_kind = stat_kind; p.accumulate = pd->accumulate; p.stat_count = stat_count;
    const dim3 grid((unsigned)nrb, (unsigned)images), block(LPROBS_NW * 64);
    if (d->dtype == PWW_DTYPE_F16) launch_attn_kernel(long_probs_kernel<f16>, grid, block, 0, st, p);
    else launch_attn_kernel(long_probs_kernel<bf16>, grid, block, 0, st, p);
    return check_hip(hipGetLastError(), "long_probs_kernel launch");
}

}  // namespace pww

PWW_LONG_API int pww_long_version(void) { return PWW_LONG_VERSION; }
PWW_LONG_API const char *pww_long_last_error(void) { return pww::last_error(); }

PWW_LONG_API int pww_long_qk_parts(const void *q, const void *k, const float *gate, const pww_attn_desc_t *desc, int32_t stat_kind, int32_t gated_images,
                                   double *partials, size_t partials_bytes, void *stream) {
    return pww::long_qk_parts(q, k, gate, desc, stat_kind, gated_images, partials, partials_bytes, static_cast<hipStream_t>(stream));
}

PWW_LONG_API int32_t pww_long_qk_parts_count(const pww_attn_desc_t *desc) { return pww::long_qk_parts_count(desc); }

PWW_LONG_API int pww_long_cross_attn_fwd_parts(const void *q, const void *k, const void *v, void *o, const float *bias, int32_t stat_kind, float coeff_scalar,
                                               const float *gate, const pww_attn_desc_t *desc, const double *partials, int32_t nparts, double *stats_out,
                                               const pww_cross_opts_t *opts, void *stream) {
    return pww::long_cross_attn(q, k, v, o, bias, stat_kind, coeff_scalar, gate, desc, partials, nparts, stats_out, opts, static_cast<hipStream_t>(stream));
}

PWW_LONG_API int pww_long_cross_attn_probs(const void *q, const void *k, const float *bias, const double *stats, int32_t stat_kind, double stat_count,
                                           float coeff_scalar, const float *gate, const pww_attn_desc_t *desc, const pww_cross_opts_t *opts, float *out,
                                           const pww_probs_desc_t *pdesc, void *stream) {
    return pww::long_probs(q, k, bias, stats, stat_kind, stat_count, coeff_scalar, gate, desc, opts, out, pdesc, static_cast<hipStream_t>(stream));
}

PWW_LONG_API int pww_long_profile_arm(void) {
    std::lock_guard<std::mutex> lock(pww::g_long_prof_mutex);
    if (!pww::g_long_ev[0]) {
        if (pww::check_hip(hipEventCreate(&pww::g_long_ev[0]), "hipEventCreate") || pww::check_hip(hipEventCreate(&pww::g_long_ev[1]), "hipEventCreate")) return PWW_EHIP;
    }
    pww::g_long_used = false;
    pww::g_long_armed = true;
    return PWW_OK;
}

PWW_LONG_API int pww_long_profile_elapsed_us(float *us) {
    hipEvent_t e0, e1;
    {
        std::lock_guard<std::mutex> lock(pww::g_long_prof_mutex);
        if (!us || !pww::g_long_used) { pww::set_error("pww_long_profile_elapsed_us: no launch was stamped since pww_long_profile_arm"); return PWW_EINVAL; }
        e0 = pww::g_long_ev[0]; e1 = pww::g_long_ev[1];
    }
    if (int rc = pww::check_hip(hipEventSynchronize(e1), "hipEventSynchronize")) return rc;
    float ms = 0.f;
    if (int rc = pww::check_hip(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime")) return rc;
    *us = ms * 1e3f;
    return PWW_OK;
}
