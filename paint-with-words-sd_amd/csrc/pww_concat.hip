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
//   pww_concat_convtail_fwd     convtail_kernel of pww_conv_tail.hip with the tail's input in two parts: tail slab t reads x1 (pitch C1)
//                               when 64 t < C1, else x2 (pitch C2, channel 64 t - C1), by wave-uniform selects like the body / tail choice.
//
// Launch form, slab and apply sizes (cat_gn_plan) and tile, K order, split boundaries, fold and TAIL_TUNED (cat_tail_plan) are those of the
// one-source entry points for C = C1 + C2: the results are BITWISE those of pww_group_norm_fwd / pww_convtail_fwd on the concatenated
// tensor (tests/test_concat_gpu.py holds every form, tile width and split to torch.equal). The kernels are WRITTEN AGAIN here, as in
// pww_linear.hip and pww_conv_tail.hip: a header shared with pww_norm.hip / pww_conv_tail.hip would move the register allocation and the
// wait counts of their code objects, and those are what their measured times rest on. A change to either plan there is a change here.
//
// Kernarg preload (14 dwords): the GroupNorm kernels carry x1, x2, the partials' pointer (the apply kernel's first loads), C1, C2, HW, G,
// cg, nslab, slab_px and apply_px hot -- what a wave needs to issue its first loads; gamma, beta, y and eps travel in the cold struct
// (B is the grid's y extent and is not passed). The tail kernel carries x, w, out, M, N, Cin, C1, C2, H, W hot (13 dwords); the two parts'
// pointers are first needed after 9 Cin / 64 slabs (or at once in a split that starts in the tail, whose prologue waits for the cold
// struct anyway for nsplit), so they stay cold beside wsc and the biases.
#define PWW_SIDE_LIB "libpww_hip_concat"
#include "pww_side_host.h"
#include "../../include/pww_hip_concat.h"

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

// ==== conv2 + shortcut over two sources (pww_conv_tail.hip) ============================================================================
constexpr int CT_BM = 128, CT_THREADS = 256;
constexpr int CT_PF = 2;        // K-slabs of global loads in flight while one is computed

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// cold kernel arguments. nmain = 9 Cin / 64 slabs of the 3 x 3 gather, ntail = (C1 + C2) / 64 of the shortcut, the first C1 / 64 of them in x1
struct CatTailCold {
    const void *x1, *x2, *wsc, *bias, *bias2;
    int nsplit, nmain, ntail;
    int through;            // split launches: the partials are stored write-through (pww_common.h: store_partial_through)
};

__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

template <typename T>
__device__ __forceinline__ void epilogue4(const f32x4 &a, const CatTailCold &cold, T *y, long off, int n) {
    typedef typename Vec<T>::v4 V4;
    const V4 b = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias) + n);
    const V4 b2 = *reinterpret_cast<const V4 *>(reinterpret_cast<const T *>(cold.bias2) + n);
    V4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)(a[j] + (float)b[j] + (float)b2[j]);
    *reinterpret_cast<V4 *>(y + off) = o;
}

template <typename T, int BN>
__global__ void __launch_bounds__(CT_THREADS, 2) cat_tail_kernel(const T *__restrict__ x, const T *__restrict__ w, void *__restrict__ out, int M, int N,
                                                                 int Cin, int C1, int C2, int H, int W, const CatTailCold cold) {
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
    const bool split = cold.nsplit > 1;
    const int tile = bid / cold.nsplit, ks = bid - tile * cold.nsplit;
    const int tm = tile % ntm, tn = tile / ntm;
    const int nmain = cold.nmain, nslab = nmain + cold.ntail;
    const int s_begin = (int)((long)ks * nslab / cold.nsplit), s_end = (int)((long)(ks + 1) * nslab / cold.nsplit);
    const int K9 = 9 * Cin, HW = H * W, Ct = C1 + C2;
    const T *__restrict__ xa = reinterpret_cast<const T *>(cold.x1);
    const T *__restrict__ xb2 = reinterpret_cast<const T *>(cold.x2);
    const T *__restrict__ w2 = reinterpret_cast<const T *>(cold.wsc);

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
    const unsigned wrow = (unsigned)(tn * BN + (tid >> 3));
    const unsigned woff_main = wrow * (unsigned)K9 + c * 8, woff_tail = wrow * (unsigned)Ct + c * 8;
    const int swz = ((c ^ ((tid >> 3) & 7)) << 4);

    u32x4 xr[PF][XL], wr[PF][WL];
    unsigned xok[PF];
    // K position of the next slab: tap 0 .. 8 of the gather, channel ci0 of it; tap 9 = the shortcut, ci0 its channel in the concatenation
    const bool tail0 = s_begin >= nmain;
    int tap = tail0 ? 9 : s_begin / (Cin >> 6);
    int ci0 = tail0 ? (s_begin - nmain) << 6 : (s_begin - tap * (Cin >> 6)) << 6;
    int kmain = s_begin * 64;
    // the tail slab's source: x1 while ci0 < C1, then x2 with its channel origin folded into the pointer (x2 - C1: only ever dereferenced
    // at ci0 >= C1), so that a tail address is `base + pixel * pitch + ci0` for both; switched by a select when ci0 reaches C1
    const bool second0 = tail0 && ci0 >= C1;
    const T *xs = second0 ? xb2 - C1 : xa;
    int ps = second0 ? C2 : C1;
    auto load = [&](int p) {
        const bool tail = tap >= 9;                         // (uniform: selects of base, pitch and tap; every load below is issued)
        const int ky = tail ? 1 : tap / 3, kx = tail ? 1 : tap - (tap / 3) * 3;
        const T *xb = tail ? xs : x;
        const T *wb = tail ? w2 : w;
        const int pitch = tail ? ps : Cin;
        const unsigned wpitch = (unsigned)(tail ? Ct : K9);
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
        const bool cross = ci0 == C1 && tail;               // (uniform: the next tail slab is the first of x2)
        xs = cross ? xb2 - C1 : xs;
        ps = cross ? C2 : ps;
    };
    auto store = [&](int p, int buf) {
        char *base = stage(buf);
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const u32x4 z = {0u, 0u, 0u, 0u};
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

    const int n = s_end - s_begin;
    load(0);
#pragma unroll
    for (int p = 1; p < PF; ++p)
        if (p < n) load(p);
    store(0, 0);
    __syncthreads();
    int i = 0;
    for (; i + 2 * PF <= n; i += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            load(p);
            compute((i + p) & 1);
            __builtin_amdgcn_sched_barrier(0);
            store((p + 1) % PF, (i + p + 1) & 1);
            __syncthreads();
        }
    }
#pragma unroll
    for (int t = 0; t < 2 * PF - 1; ++t) {
        if (i + t < n) {
            if (i + t + PF < n) load(t % PF);
            compute((i + t) & 1);
            if (i + t + 1 < n) store((t + 1) % PF, (i + t + 1) & 1);
            __syncthreads();
        }
    }

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

template <typename T>
__global__ void __launch_bounds__(256) cat_tail_fold_kernel(const float *__restrict__ ws, T *__restrict__ y, long n4, int N, long MN, const CatTailCold cold) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    const long off = q * 4;
    f32x4 a = *reinterpret_cast<const f32x4 *>(ws + off);
    for (int s = 1; s < cold.nsplit; ++s) a += *reinterpret_cast<const f32x4 *>(ws + s * MN + off);
    epilogue4<T>(a, cold, y, off, (int)(off % N));
}

// TAIL_TUNED of pww_conv_tail.hip (M, N, slabs of the gather, slabs of the shortcut = (C1 + C2) / 64, tile width, split)
struct TailTune { int M, N, nmain, ntail, bn, nsplit; };
constexpr TailTune TAIL_TUNED[] = {
    {128, 1280, 180, 40, 64, 12},
    {512, 1280, 180, 40, 128, 12}, {512, 1280, 180, 30, 128, 12}, {512, 1280, 180, 10, 128, 12},
    {2048, 640, 90, 30, 128, 6}, {2048, 640, 90, 20, 128, 6}, {2048, 640, 90, 15, 128, 6}, {2048, 640, 90, 5, 128, 6},
    {8192, 320, 45, 15, 160, 4}, {8192, 320, 45, 10, 160, 4},
};

struct TailPlan {
    int M, bn, nsplit, nmain, ntail, ntiles;
};

// plan_tail of pww_conv_tail.hip for C2 = C1 + C2, and the two parts on the 64-channel grid
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
    p->M = (int)M;
    p->nmain = 9 * d->Cin / 64;
    p->ntail = (int)(Ct / 64);
    const int nslab = p->nmain + p->ntail;
    const TailTune *tuned = nullptr;
    for (const TailTune &t : TAIL_TUNED)
        if (t.M == p->M && t.N == d->Cout && t.nmain == p->nmain && t.ntail == p->ntail) tuned = &t;
    p->bn = d->tile_n ? d->tile_n : tuned ? tuned->bn : (d->Cout % 128 == 0 ? 128 : d->Cout % 64 == 0 ? 64 : 160);
    if ((p->bn != 64 && p->bn != 128 && p->bn != 160) || d->Cout % p->bn != 0) { set_error("concat_convtail: tile_n %d does not divide Cout %d", d->tile_n, d->Cout); return false; }
    p->ntiles = (p->M + CT_BM - 1) / CT_BM * (d->Cout / p->bn);
    int ns = d->splitk;
    if (ns <= 0 && tuned && p->bn == tuned->bn) ns = tuned->nsplit;
    if (ns <= 0) {
        ns = (480 + p->ntiles / 2) / p->ntiles;
        if (ns > nslab / 8) ns = nslab / 8;
        if (ns < 1) ns = 1;
    }
    if (ns > nslab || ns > 64) { set_error("concat_convtail: split %d exceeds the %d K-slabs (or 64)", ns, nslab); return false; }
    p->nsplit = ns;
    return true;
}

template <typename T>
int cat_tail_launch(const TailPlan &p, const pww_concat_tail_desc_t *d, const void *x, const void *w, const CatTailCold &cold, void *y, void *ws,
                    hipStream_t stream) {
    const T *xt = static_cast<const T *>(x), *wt = static_cast<const T *>(w);
    const int N = d->Cout;
    const dim3 grid(p.ntiles * p.nsplit), block(CT_THREADS);
    void *out = p.nsplit == 1 ? y : ws;
    if (p.bn == 160) {
        constexpr size_t lds = 2 * (CT_BM + 160) * 128;
        static thread_local LdsRaised raised;       // (of cat_tail_kernel<T, 160>: this function is instantiated per T)
        if (raise_lds_limit(cat_tail_kernel<T, 160>, lds, raised)) return PWW_EHIP;
        launch_timed(cat_tail_kernel<T, 160>, grid, block, lds, stream, xt, wt, out, p.M, N, d->Cin, d->C1, d->C2, d->H, d->W, cold);
    } else if (p.bn == 128) launch_timed(cat_tail_kernel<T, 128>, grid, block, 0, stream, xt, wt, out, p.M, N, d->Cin, d->C1, d->C2, d->H, d->W, cold);
    else launch_timed(cat_tail_kernel<T, 64>, grid, block, 0, stream, xt, wt, out, p.M, N, d->Cin, d->C1, d->C2, d->H, d->W, cold);
    if (p.nsplit == 1) return check_hip(hipGetLastError(), "concat_convtail launch");
    const long MN = (long)p.M * N, n4 = MN / 4;
    launch_timed(cat_tail_fold_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, static_cast<const float *>(ws), static_cast<T *>(y), n4,
                 N, MN, cold);
    return check_hip(hipGetLastError(), "concat_convtail fold launch");
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
    return p.nsplit > 1 ? (size_t)p.nsplit * p.M * d->Cout * sizeof(float) : 0;
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
    const size_t need = p.nsplit > 1 ? (size_t)p.nsplit * p.M * d->Cout * sizeof(float) : 0;
    if (need && (!workspace || !aligned16(workspace) || workspace_bytes < need)) {
        set_error("concat_convtail: split %d needs a 16-byte aligned workspace of %zu bytes (got %zu)", p.nsplit, need, workspace_bytes);
        return PWW_EINVAL;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    const CatTailCold cold{x1, x2, wsc, bias, bias2, p.nsplit, p.nmain, p.ntail, need ? partial_stores_through(need) : 0};
    if (d->dtype == PWW_DTYPE_F16) return cat_tail_launch<f16>(p, d, x, w, cold, y, workspace, stream);
    return cat_tail_launch<bf16>(p, d, x, w, cold, y, workspace, stream);
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
