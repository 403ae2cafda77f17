// The two readers of `torch.cat([x1, x2], dim=1)` in an up block of the UNet, reading the two halves where they lie (libpww_hip_concat.so,
// include/pww_hip_concat.h). Every up-block ResnetBlock2D gets the concatenation of the running tensor and a skip tensor as its input; that
// tensor has exactly two readers -- norm1 of the block and the centre-tap slabs of the 1 x 1 shortcut inside conv2's kernel -- and both
// already choose a source address without a branch. Here each takes TWO sources, so the copy (12 launches, 63 MB written and read again per
// forward at 2 rows) goes away:
//
//   pww_concat_group_norm_fwd   the channels_last kernels of pww_norm.hip (gn_group_nhwc, gn_moments_nhwc + gn_apply_nhwc at 256 and 512
//                               threads), `pre` / `add` left out (norm1 has neither). A thread's piece (4 or 8 channels) lies wholly in
//                               one source when C1 and C2 are multiples of 8: it selects base pointer, row pitch and channel offset ONCE,
//                               in front of its first load. Nothing else moves: no load under a condition, the same loads in flight, the
//                               same summation order, fp32 / fp64 split and f16 pivot. A group may straddle the boundary.
//   pww_concat_convtail_fwd     the kernel of pww_convtail_fwd (pww_shortcut_gemm.h) with the tail's input in two parts: tail slab t reads
//                               x1 (pitch C1) when 64 t < C1, else x2 (pitch C2, channel 64 t - C1), by wave-uniform selects like the body /
//                               tail choice.
//
// Launch form, slab and apply sizes (cat_gn_plan) and tile, K order, split boundaries, fold and TAIL_TUNED (cat_tail_plan) are those of the
// one-source entry points for C = C1 + C2: the results are BITWISE those of pww_group_norm_fwd / pww_convtail_fwd on the concatenated
// tensor (tests/test_concat_gpu.py holds every form, tile width and split to torch.equal). The GroupNorm kernels are written again here,
// as in pww_linear.hip: they differ from those of pww_norm.hip in kernarg layout, in the `pre` / `add` code and in the written-out
// v_fma_mixlo_f16, and a header shared with that unit would move its code objects; a change to its plan is a change to cat_gn_plan. The
// conv2 + shortcut kernel is NOT a copy: it is the one `__global__` template of pww_shortcut_gemm.h, instantiated here with two parts and
// this unit's cold struct, and in pww_conv_tail.hip with one. Sharing it that way leaves all sixteen code objects of the two units as
// they were; a `__device__` body behind two `__global__` wrappers did not (profiles/shortcut_gemm.md). Plan, fold and launch come with it.
//
// Kernarg preload (14 dwords): the GroupNorm kernels carry x1, x2, the partials' pointer (the apply kernel's first loads), C1, C2, HW, G,
// cg, nslab, slab_px and apply_px hot -- what a wave needs to issue its first loads; gamma, beta, y and eps travel in the cold struct
// (B is the grid's y extent and is not passed). The tail kernel carries x, w, out, M, N, Cin, C1, C2, H, W hot (13 dwords); the two parts'
// pointers are first needed after 9 Cin / 64 slabs (or at once in a split that starts in the tail, whose prologue waits for the cold
// struct anyway for nsplit), so they stay cold beside wsc and the biases.
#define PWW_SIDE_LIB "libpww_hip_concat"
#include "pww_side_host.h"
#include "../../include/pww_hip_concat.h"
#include "pww_shortcut_gemm.h"

#define PWW_CONCAT_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

// ==== GroupNorm over two sources (pww_norm.hip, NHWC) ==================================================================================
constexpr int GN_NT = 256;
constexpr int GN_UN = 8;                      // loads a thread keeps in flight in the streaming loops
constexpr int GN_MAX_SLABS = 64;              // partials per (image, group)
constexpr int GN_GROUP_PIECES = 24;           // single-launch form: pieces a thread keeps in registers

struct CatGnCold {
    const void *gamma, *beta;
    void *y;
    float eps;
};
#define CG_KARGS const void *x1_, const void *x2_, double *partial_, int C1_, int C2_, int HW_, int G_, int cg_, int nslab_, int slab_px_, int apply_px_, const CatGnCold cold_
struct CatGnParams {
    const void *x1, *x2, *gamma, *beta;
    void *y;
    double *partial;
    int C1, C2, C, HW, G, cg, nslab, slab_px, apply_px;
    float eps;
};
#define CG_UNPACK const CatGnParams p = {x1_, x2_, cold_.gamma, cold_.beta, cold_.y, partial_, C1_, C2_, C1_ + C2_, HW_, G_, cg_, nslab_, slab_px_, apply_px_, cold_.eps};
#define CG_LARGS(p) p.x1, p.x2, p.partial, p.C1, p.C2, p.HW, p.G, p.cg, p.nslab, p.slab_px, p.apply_px, CatGnCold{p.gamma, p.beta, p.y, p.eps}

typedef double f64x2 __attribute__((ext_vector_type(2)));

template <typename T> __device__ __forceinline__ float round_to(float v) { return (float)(T)v; }

template <typename T> struct GnPivot { static constexpr bool on = false; };
template <> struct GnPivot<f16> { static constexpr bool on = true; };
__device__ __forceinline__ void unpivot(double &S, double &Q, double s, double q, double c, double n) {
    S += s + n * c;
    Q += q + 2.0 * c * s + n * c * c;
}

// T(fma(a, h, b)). float16: every code object of pww_norm.hip does this in ONE instruction, v_fma_mixlo_f16, which rounds the exact fma to
// float16 once; here, without the `pre` / `add` code around it, the compiler picks packed fp32 fmas and a separate conversion for some of
// the kernels -- two roundings, another bit in about one output of 13 000 (measured: 33 of 442 368). The instruction is therefore written
// out, so that the two-source result does not hang on instruction selection.
template <typename T> __device__ __forceinline__ float fma_round(float a, float h, float b) { return round_to<T>(fmaf(a, h, b)); }
template <> __device__ __forceinline__ float fma_round<f16>(float a, float h, float b) {
    unsigned r;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(h), "v"(b));      // (writes the low half of r; the high half is masked off)
    return (float)__builtin_bit_cast(f16, (unsigned short)(r & 0xffffu));
}

template <typename T, int ACT> __device__ __forceinline__ float finish(float h, float a, float b) {
    float y = fma_round<T>(a, h, b);
    if (ACT == 1) y = y / (1.f + __expf(-y));
    return y;
}

__device__ __forceinline__ void mean_rstd(double S, double Q, double n, float eps, float &mean, float &rstd) {
    const double m = S / n;
    double var = Q / n - m * m;
    var = var > 0.0 ? var : 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

__device__ __forceinline__ void wg_sum(double &S, double &Q, double (*red)[2], int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { S += __shfl_down(S, off); Q += __shfl_down(Q, off); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = S; red[tid >> 6][1] = Q; }
    __syncthreads();
    S = 0.0; Q = 0.0;
#pragma unroll
    for (int w = 0; w < GN_NT / 64; ++w) { S += red[w][0]; Q += red[w][1]; }
}

// The source of the piece that starts at channel c0 of the concatenation (c0 < C1 + C2; the piece does not cross C1): its first element in
// image b, and the source's row pitch. Selects, no branch; the only thing the two-source kernels add to the one-source ones.
template <typename T>
__device__ __forceinline__ const T *cat_source(const CatGnParams &p, int b, int c0, int &pitch) {
    const bool second = c0 >= p.C1;
    pitch = second ? p.C2 : p.C1;
    const T *base = reinterpret_cast<const T *>(second ? p.x2 : p.x1);
    return base + (long)b * p.HW * pitch + (second ? c0 - p.C1 : c0);
}

template <typename T, int NT>
__global__ void __launch_bounds__(NT) cat_gn_moments(CG_KARGS) {
    CG_UNPACK
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename Vec<T>::v8 V8;
    const int tid = threadIdx.x, b = blockIdx.y, slab = blockIdx.x;
    const int CH = p.C >> 3, PL = NT / CH;
    const int pl = tid / CH, ch = tid - pl * CH;
    float *ls = reinterpret_cast<float *>(smem);                  // [PL][C] per-thread channel sums
    float *lq = ls + PL * p.C;                                    // [PL][C] ... of squares
    double *lk = reinterpret_cast<double *>(lq + PL * p.C);       // [K][G][2]

    if (pl < PL) {
        float s[8], q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
        int pitch;
        const T *x = cat_source<T>(p, b, ch * 8, pitch);
        float c = 0.f;                                            // f16: the thread's first value (its chunk's first channel)
        const int p0 = slab * p.slab_px, p1 = min(p0 + p.slab_px, p.HW);
#pragma unroll 1
        for (int px = p0 + pl; px < p1; px += GN_UN * PL) {
            V8 r[GN_UN];
#pragma unroll
            for (int u = 0; u < GN_UN; ++u) {
                const int pu = px + u * PL;
                r[u] = *reinterpret_cast<const V8 *>(x + (long)(pu < p1 ? pu : px) * pitch);
            }
            if constexpr (GnPivot<T>::on) {
                if (px == p0 + pl) c = (float)r[0][0];
            }
#pragma unroll
            for (int u = 0; u < GN_UN; ++u) {
                const bool ok = px + u * PL < p1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float h = (float)r[u][j];
                    if constexpr (GnPivot<T>::on) h -= c;
                    h = ok ? h : 0.f;
                    s[j] += h;
                    q[j] = fmaf(h, h, q[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { ls[pl * p.C + ch * 8 + j] = s[j]; lq[pl * p.C + ch * 8 + j] = q[j]; }
        if constexpr (GnPivot<T>::on) reinterpret_cast<float *>(lk + (NT / p.G) * p.G * 2)[tid] = c;      // [PL][CH] pivots behind lk
    }
    __syncthreads();
    const int K = NT / p.G, g = tid % p.G, k = tid / p.G;
    if (k < K) {
        double S = 0.0, Q = 0.0;
        const int n = PL * p.cg;
        for (int e = k; e < n; e += K) {
            const int r = e / p.cg, c = g * p.cg + (e - r * p.cg);
            if constexpr (GnPivot<T>::on) {
                const float *lc = reinterpret_cast<const float *>(lk + K * p.G * 2);
                const int p0 = slab * p.slab_px, p1 = min(p0 + p.slab_px, p.HW);
                const int cnt = p0 + r < p1 ? (p1 - p0 - r + PL - 1) / PL : 0;
                unpivot(S, Q, (double)ls[r * p.C + c], (double)lq[r * p.C + c], (double)lc[r * CH + (c >> 3)], (double)cnt);
            } else {
                S += (double)ls[r * p.C + c]; Q += (double)lq[r * p.C + c];
            }
        }
        lk[(k * p.G + g) * 2] = S; lk[(k * p.G + g) * 2 + 1] = Q;
    }
    __syncthreads();
    if (tid < p.G) {
        double S = 0.0, Q = 0.0;
        for (int r = 0; r < K; ++r) { S += lk[(r * p.G + tid) * 2]; Q += lk[(r * p.G + tid) * 2 + 1]; }
        f64x2 v; v[0] = S; v[1] = Q;
        reinterpret_cast<f64x2 *>(p.partial)[((long)b * p.nslab + slab) * p.G + tid] = v;
    }
}

template <typename T, int ACT, int NT>
__global__ void __launch_bounds__(NT) cat_gn_apply(CG_KARGS) {
    CG_UNPACK
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename Vec<T>::v8 V8;
    constexpr int NPART = 8;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int CH = p.C >> 3, PL = NT / CH;
    const int pl = tid / CH, ch = tid - pl * CH;
    const bool active = pl < PL;
    double *lk = reinterpret_cast<double *>(smem);                  // [K][G][2]
    const int K = NT / p.G, g = tid % p.G, k = tid / p.G;
    float *stat = reinterpret_cast<float *>(lk + K * p.G * 2);       // [G][2] mean, rstd

    f64x2 part[NPART];
#pragma unroll
    for (int i = 0; i < NPART; ++i) {
        const int sl = k + i * K;
        part[i] = reinterpret_cast<const f64x2 *>(p.partial)[((long)b * p.nslab + (k < K && sl < p.nslab ? sl : 0)) * p.G + g];
    }
    const int c0 = ch * 8;
    V8 gv = zero8<V8>(), bv = zero8<V8>();
    int pitch;
    const T *x = cat_source<T>(p, b, c0, pitch);
    T *y = reinterpret_cast<T *>(p.y) + (long)b * p.HW * p.C + c0;
    const int p0 = blockIdx.x * p.apply_px, p1 = min(p0 + p.apply_px, p.HW);
    V8 r[GN_UN];
    if (active) {
        if (p.gamma) gv = *reinterpret_cast<const V8 *>(reinterpret_cast<const T *>(p.gamma) + c0);
        if (p.beta) bv = *reinterpret_cast<const V8 *>(reinterpret_cast<const T *>(p.beta) + c0);
#pragma unroll
        for (int u = 0; u < GN_UN; ++u) {
            const int pu = p0 + pl + u * PL;
            r[u] = *reinterpret_cast<const V8 *>(x + (long)(pu < p1 ? pu : p0) * pitch);
        }
    }
    if (k < K) {
        double S = 0.0, Q = 0.0;
#pragma unroll
        for (int i = 0; i < NPART; ++i)
            if (k + i * K < p.nslab) { S += part[i][0]; Q += part[i][1]; }
        lk[(k * p.G + g) * 2] = S; lk[(k * p.G + g) * 2 + 1] = Q;
    }
    __syncthreads();
    if (tid < p.G) {
        double S = 0.0, Q = 0.0;
        for (int rr = 0; rr < K; ++rr) { S += lk[(rr * p.G + tid) * 2]; Q += lk[(rr * p.G + tid) * 2 + 1]; }
        float mean, rstd;
        mean_rstd(S, Q, (double)p.cg * (double)p.HW, p.eps, mean, rstd);
        stat[tid * 2] = mean; stat[tid * 2 + 1] = rstd;
    }
    __syncthreads();
    if (!active) return;
    float a[8], bb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int gg = (c0 + j) / p.cg;
        a[j] = stat[gg * 2 + 1] * (p.gamma ? (float)gv[j] : 1.f);
        bb[j] = (p.beta ? (float)bv[j] : 0.f) - a[j] * stat[gg * 2];
    }
    for (int px = p0 + pl; px < p1; px += GN_UN * PL) {
        if (px != p0 + pl) {
#pragma unroll
            for (int u = 0; u < GN_UN; ++u) {
                const int pu = px + u * PL;
                r[u] = *reinterpret_cast<const V8 *>(x + (long)(pu < p1 ? pu : px) * pitch);
            }
        }
#pragma unroll
        for (int u = 0; u < GN_UN; ++u) {
            V8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (T)finish<T, ACT>((float)r[u][j], a[j], bb[j]);
            if (px + u * PL < p1) *reinterpret_cast<V8 *>(y + (long)(px + u * PL) * p.C) = o;
        }
    }
}

// One launch, workgroup = (group, image): thread t owns the 4-channel piece t % ppp of every PLs-th pixel of the group
template <typename T, int ACT>
__global__ void __launch_bounds__(GN_NT) cat_gn_group(CG_KARGS) {
    CG_UNPACK
    typedef T TV __attribute__((ext_vector_type(4)));
    __shared__ double red[GN_NT / 64][2];
    const int tid = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
    const int ppp = p.cg >> 2, PLs = GN_NT / ppp;
    const int pl = tid / ppp, sub = tid - pl * ppp;
    const bool active = pl < PLs;
    const int pc = pl < p.HW ? pl : 0;            // the pixel a masked piece loads instead: one of the image (HW < PLs: pl itself is none)
    const int c0 = g * p.cg + sub * 4;
    int pitch;
    const T *x = cat_source<T>(p, b, c0, pitch);
    T *y = reinterpret_cast<T *>(p.y) + (long)b * p.HW * p.C + c0;
    TV raw[GN_GROUP_PIECES];
    const TV z = {(T)0.f, (T)0.f, (T)0.f, (T)0.f};
    TV gv = z, bv = z;
    if (active) {
#pragma unroll
        for (int j = 0; j < GN_GROUP_PIECES; ++j) {
            const int px = pl + j * PLs;
            raw[j] = *reinterpret_cast<const TV *>(x + (long)(px < p.HW ? px : pc) * pitch);
        }
        if (p.gamma) gv = *reinterpret_cast<const TV *>(reinterpret_cast<const T *>(p.gamma) + c0);
        if (p.beta) bv = *reinterpret_cast<const TV *>(reinterpret_cast<const T *>(p.beta) + c0);
    }
    float v[GN_GROUP_PIECES][4];
    float s = 0.f, q = 0.f, c = 0.f;
    int cnt = 0;                                  // f16: the thread's values, summed around its first one
    if (active) {
#pragma unroll
        for (int j = 0; j < GN_GROUP_PIECES; ++j) {
            const bool ok = pl + j * PLs < p.HW;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float h = (float)raw[j][e];
                h = ok ? h : 0.f;
                v[j][e] = h;
                if constexpr (GnPivot<T>::on) {
                    if (j == 0 && e == 0) c = h;
                    h = ok ? h - c : 0.f;
                }
                s += h;
                q = fmaf(h, h, q);
            }
            if constexpr (GnPivot<T>::on) cnt += ok ? 4 : 0;
        }
    }
    double S = (double)s, Q = (double)q;
    if constexpr (GnPivot<T>::on) { S = 0.0; Q = 0.0; unpivot(S, Q, (double)s, (double)q, (double)c, (double)cnt); }
    wg_sum(S, Q, red, tid);
    float mean, rstd;
    mean_rstd(S, Q, (double)p.cg * (double)p.HW, p.eps, mean, rstd);      // (every thread: no second barrier)
    if (!active) return;
    float a[4], bb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a[e] = rstd * (p.gamma ? (float)gv[e] : 1.f);
        bb[e] = (p.beta ? (float)bv[e] : 0.f) - a[e] * mean;
    }
#pragma unroll
    for (int j = 0; j < GN_GROUP_PIECES; ++j) {
        const int px = pl + j * PLs;
        if (px < p.HW) {
            TV o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (T)finish<T, ACT>(v[j][e], a[e], bb[e]);
            *reinterpret_cast<TV *>(y + (long)px * p.C) = o;
        }
    }
}

struct CatGnPlan { int nslab, slab_px, apply_px, nt; bool group; size_t partial_bytes, lds_m, lds_a; };

bool desc_ok(const void *d, uint32_t size, size_t want, const char *what) {
    if (d && size >= want) return true;
    set_error("%s: descriptor missing or older than this library (size %u)", what, d ? size : 0u);
    return false;
}

// gn_plan of pww_norm.hip for a channels_last tensor of C1 + C2 channels, and the two parts on the 8-channel grid
bool cat_gn_plan(const pww_concat_gn_desc_t *d, CatGnPlan &pl) {
    const long C = (long)d->C1 + d->C2;
    const bool ok = d->B >= 1 && d->B <= 65535 && d->C1 >= 8 && d->C2 >= 8 && d->C1 % 8 == 0 && d->C2 % 8 == 0 && C <= 4096 && d->HW >= 8 && d->HW % 8 == 0
                    && d->G >= 1 && d->G <= 32 && C % d->G == 0 && (d->dtype == PWW_DTYPE_F16 || d->dtype == PWW_DTYPE_BF16)
                    && (d->act == PWW_ACT_NONE || d->act == PWW_ACT_SILU) && (long)d->B * d->HW * C < (1L << 40);
    if (!ok) {
        set_error("concat_group_norm: unsupported (dtype %d B %d C1 %d C2 %d HW %d G %d act %d): C1, C2 and HW multiples of 8, (C1 + C2) %% G == 0, "
                  "G <= 32, C1 + C2 <= 4096", d->dtype, d->B, d->C1, d->C2, d->HW, d->G, d->act);
        return false;
    }
    pl = CatGnPlan();
    const int Ct = (int)C, cg = Ct / d->G, CH = Ct / 8;
    pl.nt = CH <= 256 ? 256 : 512;
    const int PL = pl.nt / CH;
    if (cg % 4 == 0 && cg / 4 <= GN_NT) {
        const int PLs = GN_NT / (cg / 4);
        pl.group = (d->HW + PLs - 1) / PLs <= GN_GROUP_PIECES;
    }
    int px = (d->HW + GN_MAX_SLABS - 1) / GN_MAX_SLABS;
    if (px < GN_UN * PL) px = GN_UN * PL;
    if (px > d->HW) px = d->HW;
    pl.slab_px = px;
    pl.nslab = (d->HW + px - 1) / px;
    int want = (512 + d->B - 1) / d->B;
    int apx = (d->HW + want - 1) / want;
    if (apx < GN_UN * PL) apx = GN_UN * PL;
    if (apx > d->HW) apx = d->HW;
    pl.apply_px = apx;
    pl.partial_bytes = (size_t)d->B * pl.nslab * d->G * 2 * sizeof(double);
    const size_t lk = (size_t)(pl.nt / d->G) * d->G * 2 * sizeof(double);
    pl.lds_m = (size_t)2 * PL * Ct * sizeof(float) + lk + (d->dtype == PWW_DTYPE_F16 ? (size_t)pl.nt * sizeof(float) : 0);      // (+ the pivots)
    pl.lds_a = lk + (size_t)d->G * 2 * sizeof(float);
    return true;
}

template <typename T>
int cat_gn_launch(const CatGnParams &p, const pww_concat_gn_desc_t *d, const CatGnPlan &pl, hipStream_t stream) {
    const bool silu = d->act == PWW_ACT_SILU;
    if (pl.group) {
        const dim3 grid(d->G, d->B);
        if (silu) hipLaunchKernelGGL((cat_gn_group<T, 1>), grid, dim3(GN_NT), 0, stream, CG_LARGS(p));
        else hipLaunchKernelGGL((cat_gn_group<T, 0>), grid, dim3(GN_NT), 0, stream, CG_LARGS(p));
        return check_hip(hipGetLastError(), "concat_group_norm launch");
    }
    const dim3 gm(pl.nslab, d->B), ga((d->HW + pl.apply_px - 1) / pl.apply_px, d->B);
    if (pl.nt == 256) {
        hipLaunchKernelGGL((cat_gn_moments<T, 256>), gm, dim3(256), pl.lds_m, stream, CG_LARGS(p));
        if (silu) hipLaunchKernelGGL((cat_gn_apply<T, 1, 256>), ga, dim3(256), pl.lds_a, stream, CG_LARGS(p));
        else hipLaunchKernelGGL((cat_gn_apply<T, 0, 256>), ga, dim3(256), pl.lds_a, stream, CG_LARGS(p));
    } else {
        hipLaunchKernelGGL((cat_gn_moments<T, 512>), gm, dim3(512), pl.lds_m, stream, CG_LARGS(p));
        if (silu) hipLaunchKernelGGL((cat_gn_apply<T, 1, 512>), ga, dim3(512), pl.lds_a, stream, CG_LARGS(p));
        else hipLaunchKernelGGL((cat_gn_apply<T, 0, 512>), ga, dim3(512), pl.lds_a, stream, CG_LARGS(p));
    }
    return check_hip(hipGetLastError(), "concat_group_norm launch");
}

// ==== conv2 + shortcut over two sources (pww_shortcut_gemm.h) ===========================================================================
// cold kernel arguments. nmain = 9 Cin / 64 slabs of the 3 x 3 gather, ntail = (C1 + C2) / 64 of the shortcut, the first C1 / 64 of them in x1
struct CatTailCold {
    const void *x1, *x2, *wsc, *bias, *bias2;
    int nsplit, nmain, ntail;
    int through;            // split launches: the partials are stored write-through (pww_common.h: store_partial_through)
};

// the checks of pww_convtail_fwd for C2 = C1 + C2 with the two parts on the 64-channel grid, then the shared plan
bool cat_tail_plan(const pww_concat_tail_desc_t *d, TailPlan *p) {
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 64 || d->Cin % 64 != 0 || d->C1 < 64
        || d->C1 % 64 != 0 || d->C2 < 64 || d->C2 % 64 != 0 || d->Cout < 64 || (d->Cout % 64 != 0 && d->Cout % 160 != 0) || d->Cin > 65536 || d->C1 > 32768
        || d->C2 > 32768 || d->Cout > 65536) {
        set_error("concat_convtail: unsupported (dtype %d B %d %dx%d Cin %d C1 %d C2 %d Cout %d): Cin, C1 and C2 multiples of 64, Cout of 64 or 160", d->dtype,
                  d->B, d->H, d->W, d->Cin, d->C1, d->C2, d->Cout);
        return false;
    }
    const long M = (long)d->B * d->H * d->W, Ct = (long)d->C1 + d->C2;
    if (M * d->Cin >= (1L << 31) || M * Ct >= (1L << 31) || M * d->Cout >= (1L << 31) || 9L * d->Cin * d->Cout >= (1L << 31) || Ct * d->Cout >= (1L << 31)) {
        set_error("concat_convtail: tensor of 2^31 elements or more");
        return false;
    }
    return plan_tail("concat_convtail", (int)M, 9 * d->Cin / 64, (int)(Ct / 64), d->Cout, d->tile_n, d->splitk, p);
}

}  // namespace

size_t concat_group_norm_workspace_bytes(const pww_concat_gn_desc_t *d) {
    CatGnPlan pl;
    if (!desc_ok(d, d ? d->size : 0u, sizeof(pww_concat_gn_desc_t), "concat_group_norm") || !cat_gn_plan(d, pl)) return 0;
    return pl.group ? 16 : pl.partial_bytes;
}

int concat_group_norm_fwd(const void *x1, const void *x2, const void *gamma, const void *beta, void *y, const pww_concat_gn_desc_t *d, void *workspace,
                          size_t workspace_bytes, hipStream_t stream) {
    if (!desc_ok(d, d ? d->size : 0u, sizeof(pww_concat_gn_desc_t), "concat_group_norm")) return PWW_EINVAL;
    CatGnPlan pl;
    if (!cat_gn_plan(d, pl)) return PWW_ENOTSUP;
    if (!x1 || !x2 || !y || !workspace) { set_error("concat_group_norm: x1, x2, y and workspace are required"); return PWW_EINVAL; }
    if (!aligned16(x1) || !aligned16(x2) || !aligned16(y) || !aligned16(workspace) || !aligned16(gamma) || !aligned16(beta)) {
        set_error("concat_group_norm: pointers must be 16-byte aligned");
        return PWW_EINVAL;
    }
    const size_t need = pl.group ? 16 : pl.partial_bytes;
    if (workspace_bytes < need) { set_error("concat_group_norm: workspace of %zu bytes, need %zu", workspace_bytes, need); return PWW_EINVAL; }
    if (!arch_ok()) return PWW_ENOTSUP;
    CatGnParams p;
    p.x1 = x1; p.x2 = x2; p.gamma = gamma; p.beta = beta; p.y = y;
    p.partial = static_cast<double *>(workspace);
    p.C1 = d->C1; p.C2 = d->C2; p.C = d->C1 + d->C2; p.HW = d->HW; p.G = d->G; p.cg = p.C / d->G;
    p.nslab = pl.nslab; p.slab_px = pl.slab_px; p.apply_px = pl.apply_px;
    p.eps = d->eps;
    return d->dtype == PWW_DTYPE_F16 ? cat_gn_launch<f16>(p, d, pl, stream) : cat_gn_launch<bf16>(p, d, pl, stream);
}

size_t concat_convtail_workspace_bytes(const pww_concat_tail_desc_t *d) {
    TailPlan p;
    if (!desc_ok(d, d ? d->size : 0u, sizeof(pww_concat_tail_desc_t), "concat_convtail") || !cat_tail_plan(d, &p)) return 0;
    return tail_workspace_bytes(p, d->Cout);
}

int concat_convtail_fwd(const void *x, const void *w, const void *x1, const void *x2, const void *wsc, const void *bias, const void *bias2, void *y,
                        const pww_concat_tail_desc_t *d, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!desc_ok(d, d ? d->size : 0u, sizeof(pww_concat_tail_desc_t), "concat_convtail")) return PWW_EINVAL;
    TailPlan p;
    if (!cat_tail_plan(d, &p)) return PWW_ENOTSUP;
    if (!x || !w || !x1 || !x2 || !wsc || !bias || !bias2 || !y) { set_error("concat_convtail: x, w, x1, x2, wsc, bias, bias2 and y are required"); return PWW_EINVAL; }
    if (!aligned16(x) || !aligned16(w) || !aligned16(x1) || !aligned16(x2) || !aligned16(wsc) || !aligned16(y) || (reinterpret_cast<uintptr_t>(bias) & 7)
        || (reinterpret_cast<uintptr_t>(bias2) & 7)) {
        set_error("concat_convtail: x, w, x1, x2, wsc, y must be 16-byte aligned, the biases 8-byte aligned");
        return PWW_EINVAL;
    }
    const size_t need = tail_workspace_bytes(p, d->Cout);
    if (need && (!workspace || !aligned16(workspace) || workspace_bytes < need)) {
        set_error("concat_convtail: split %d needs a 16-byte aligned workspace of %zu bytes (got %zu)", p.nsplit, need, workspace_bytes);
        return PWW_EINVAL;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    const CatTailCold cold{x1, x2, wsc, bias, bias2, 0, 0, 0, 0};       // (the plan's half is filled in by the launch)
    if (d->dtype == PWW_DTYPE_F16) return tail_launch<f16>("concat_convtail", p, x, w, cold, y, workspace, d->Cout, d->Cin, d->H, d->W, stream, d->C1, d->C2);
    return tail_launch<bf16>("concat_convtail", p, x, w, cold, y, workspace, d->Cout, d->Cin, d->H, d->W, stream, d->C1, d->C2);
}

}  // namespace pww

PWW_CONCAT_API int pww_concat_version(void) { return PWW_CONCAT_VERSION; }
PWW_CONCAT_API const char *pww_concat_last_error(void) { return pww::last_error(); }
PWW_CONCAT_API size_t pww_concat_group_norm_workspace_bytes(const pww_concat_gn_desc_t *desc) { return pww::concat_group_norm_workspace_bytes(desc); }
PWW_CONCAT_API int pww_concat_group_norm_fwd(const void *x1, const void *x2, const void *gamma, const void *beta, void *y, const pww_concat_gn_desc_t *desc,
                                             void *workspace, size_t workspace_bytes, void *stream) {
    return pww::concat_group_norm_fwd(x1, x2, gamma, beta, y, desc, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
PWW_CONCAT_API size_t pww_concat_convtail_workspace_bytes(const pww_concat_tail_desc_t *desc) { return pww::concat_convtail_workspace_bytes(desc); }
PWW_CONCAT_API int pww_concat_convtail_fwd(const void *x, const void *w, const void *x1, const void *x2, const void *wsc, const void *bias, const void *bias2,
                                           void *y, const pww_concat_tail_desc_t *desc, void *workspace, size_t workspace_bytes, void *stream) {
    return pww::concat_convtail_fwd(x, w, x1, x2, wsc, bias, bias2, y, desc, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
