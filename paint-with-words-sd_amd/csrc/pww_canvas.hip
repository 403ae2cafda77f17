// Canvases larger than the UNet's window (include/pww_hip_canvas.h): the canvas latent is denoised as overlapping windows, and the per-pixel
// weighted mean of the windows' noise predictions takes one scheduler step on the canvas. Two launches around the UNet evaluation of a step:
//
//   canvas_gather_kernel     canvas fp32 [C][Hc][Wc] -> T [copies][n_w][C][h][w]: every window's crop, divided by the scheduler's input
//                            scale (one fp32 division) and rounded to the UNet's type, written once per row class. Grid: (lanes of one
//                            window, window). A lane owns 8 consecutive elements of a window row (4-byte loads -- an odd origin makes the
//                            canvas rows unaligned -- and one 16-byte store per copy) or, where w or the address does not allow that, one.
//   canvas_combine_kernel    the UNet's output T [(K + 2)][n_w][C][h][w] -> fp32 [C][Hc][Wc], gather form: a lane owns 8 consecutive canvas
//                            pixels (or one) and walks the windows that cover them in ascending window index; the window's weight p and,
//                            with region prompts, its K + 1 blend coefficients are formed once per pixel and window and reused over the
//                            channels (four accumulators per pixel: the channels are walked four at a time). No atomics: a canvas pixel
//                            is written by the one lane that owns it.
//
// The window origins travel in the kernel arguments (at most 64 per axis); every index into them is uniform over the wave.
//
// The arithmetic is fp32, one IEEE operation per step in the order include/pww_hip_canvas.h writes down; the unit is compiled with
// -ffp-contract=off (build.py PER_FILE_FLAGS) and spells the operations as __f*_rn besides, so a CPU restatement matches bit for bit.
//
// Built as a library of its own (libpww_hip_canvas.so): the unit is self-contained, its host plumbing is pww_side_host.h, and only the
// pww_canvas_* entry points are visible (compiled with -fvisibility=hidden).
#include <math.h>
#define PWW_SIDE_LIB "libpww_hip_canvas"
#include "pww_side_host.h"
#include "../../include/pww_hip_canvas.h"

#define PWW_CANVAS_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int CV_GATHER_THREADS = 256;
constexpr int CV_COMBINE_THREADS = 64;       // small workgroups: a 64 x 256 canvas is 2048 lanes of 8 pixels, spread over 32 CUs
constexpr int CV_CB = 4;                     // channels per pass of the combine (accumulators per pixel)

struct Plan {
    int ys[PWW_CANVAS_MAX_WINDOWS], xs[PWW_CANVAS_MAX_WINDOWS];
    int ny, nx, C, Hc, Wc, h, w;
};

struct GatherArgs {
    const float *canvas;
    void *out;
    float denom;
    int copies;
    Plan p;
};

struct CombineArgs {
    const void *eps;
    const float *masks, *weights, *scales;
    float *out;
    float g;
    int K, ramp;
    Plan p;
};

template <typename T, int V> struct Pack;
template <typename T> struct Pack<T, 1> {
    static __device__ __forceinline__ void store(T *p, const T (&v)[1]) { p[0] = v[0]; }
    static __device__ __forceinline__ void load(const T *p, float (&v)[1]) { v[0] = (float)p[0]; }
    static __device__ __forceinline__ void load_f32(const float *p, float (&v)[1]) { v[0] = p[0]; }
    static __device__ __forceinline__ void store_f32(float *p, const float (&v)[1]) { p[0] = v[0]; }
};
template <typename T> struct Pack<T, 8> {
    static __device__ __forceinline__ void store(T *p, const T (&v)[8]) {
        typename Vec<T>::v8 x;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = v[j];
        *reinterpret_cast<u32x4 *>(p) = __builtin_bit_cast(u32x4, x);
    }
    static __device__ __forceinline__ void load(const T *p, float (&v)[8]) {
        const typename Vec<T>::v8 x = __builtin_bit_cast(typename Vec<T>::v8, *reinterpret_cast<const u32x4 *>(p));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)x[j];
    }
    static __device__ __forceinline__ void load_f32(const float *p, float (&v)[8]) {
        const f32x4 lo = *reinterpret_cast<const f32x4 *>(p), hi = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
    }
    static __device__ __forceinline__ void store_f32(float *p, const float (&v)[8]) {
        const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
        *reinterpret_cast<f32x4 *>(p) = lo;
        *reinterpret_cast<f32x4 *>(p + 4) = hi;
    }
};

template <typename T, int V>
__global__ void __launch_bounds__(CV_GATHER_THREADS) canvas_gather_kernel(const GatherArgs a) {
    const Plan &p = a.p;
    const int win = blockIdx.y, iy = win / p.nx, ix = win - iy * p.nx;
    const int y0 = p.ys[iy], x0 = p.xs[ix];
    const long per = (long)p.C * p.h * p.w;                      // one window image
    const long e0 = ((long)blockIdx.x * CV_GATHER_THREADS + threadIdx.x) * V;
    if (e0 >= per) return;
    // (V = 8 only when w is a multiple of 8: the lane's elements stay inside one row of the window)
    const long r = e0 / p.w;
    const int lx = (int)(e0 - r * p.w), c = (int)(r / p.h), ly = (int)(r - (long)c * p.h);
    const float *src = a.canvas + ((long)c * p.Hc + (y0 + ly)) * p.Wc + (x0 + lx);
    T v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (T)__fdiv_rn(src[j], a.denom);
    T *out = static_cast<T *>(a.out) + (long)win * per + e0;
    const long copy = (long)p.ny * p.nx * per;
    for (int cp = 0; cp < a.copies; ++cp) Pack<T, V>::store(out + cp * copy, v);
}

// r_L(l) of the header
__device__ __forceinline__ int ramp_weight(int l, int L, int ramp) {
    if (ramp == 0) return 1;
    const int edge = l < L - 1 - l ? l : L - 1 - l;
    return edge + 1 < ramp ? edge + 1 : ramp;
}

template <typename T, int V>
__global__ void __launch_bounds__(CV_COMBINE_THREADS) canvas_combine_kernel(const CombineArgs a) {
    const Plan &p = a.p;
    const long area = (long)p.Hc * p.Wc;
    const long px = ((long)blockIdx.x * CV_COMBINE_THREADS + threadIdx.x) * V;
    if (px >= area) return;
    // (V = 8 only when Wc, w and every origin of xs are multiples of 8: the lane's pixels share a canvas row and their covering windows)
    const int y = (int)(px / p.Wc), x = (int)(px - (long)y * p.Wc);
    const long plane = (long)p.h * p.w, image = (long)p.C * plane, cls = (long)p.ny * p.nx * image;      // one channel / window / row class of eps
    const T *eps = static_cast<const T *>(a.eps);
    for (int c0 = 0; c0 < p.C; c0 += CV_CB) {
        float acc[CV_CB][V], ps[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            ps[j] = 0.f;
#pragma unroll
            for (int cc = 0; cc < CV_CB; ++cc) acc[cc][j] = 0.f;
        }
        for (int iy = 0; iy < p.ny; ++iy) {
            const int ly = y - p.ys[iy];
            if (ly < 0 || ly >= p.h) continue;
            const int rh = ramp_weight(ly, p.h, a.ramp);
            for (int ix = 0; ix < p.nx; ++ix) {
                const int lx = x - p.xs[ix];
                if (lx < 0 || lx >= p.w) continue;
                const int win = iy * p.nx + ix;
                const long at = (long)ly * p.w + lx;
                float pw[V];
#pragma unroll
                for (int j = 0; j < V; ++j) pw[j] = (float)(rh * ramp_weight(lx + j, p.w, a.ramp));
                // the K + 1 coefficients of this window at the lane's pixels: c[0] = w_0 g, c[k] = w_k s_k
                float c[PWW_REGIONS_MAX + 1][V], sum[V];
#pragma unroll
                for (int k = 0; k < PWW_REGIONS_MAX; ++k) {
                    if (k < a.K) {
                        const float ak = a.weights[(long)win * a.K + k], sk = a.scales[(long)win * a.K + k];
                        float m[V];
                        Pack<T, V>::load_f32(a.masks + ((long)win * a.K + k) * plane + at, m);
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            const float wk = __fmul_rn(ak, m[j]);
                            sum[j] = k == 0 ? wk : __fadd_rn(sum[j], wk);
                            c[k + 1][j] = __fmul_rn(wk, sk);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < V; ++j) c[0][j] = a.K > 0 ? __fmul_rn(__fsub_rn(1.f, sum[j]), a.g) : a.g;
#pragma unroll
                for (int cc = 0; cc < CV_CB; ++cc) {
                    if (c0 + cc < p.C) {
                        const long base = (long)win * image + (long)(c0 + cc) * plane + at;
                        float u[V], e[V], v[V];
                        Pack<T, V>::load(eps + (long)(a.K + 1) * cls + base, u);
                        Pack<T, V>::load(eps + base, e);
#pragma unroll
                        for (int j = 0; j < V; ++j) v[j] = __fadd_rn(u[j], __fmul_rn(c[0][j], __fsub_rn(e[j], u[j])));
#pragma unroll
                        for (int k = 0; k < PWW_REGIONS_MAX; ++k) {
                            if (k < a.K) {
                                Pack<T, V>::load(eps + (long)(k + 1) * cls + base, e);
#pragma unroll
                                for (int j = 0; j < V; ++j) v[j] = __fadd_rn(v[j], __fmul_rn(c[k + 1][j], __fsub_rn(e[j], u[j])));
                            }
                        }
#pragma unroll
                        for (int j = 0; j < V; ++j) acc[cc][j] = __fadd_rn(acc[cc][j], __fmul_rn(pw[j], v[j]));
                    }
                }
#pragma unroll
                for (int j = 0; j < V; ++j) ps[j] = __fadd_rn(ps[j], pw[j]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < CV_CB; ++cc) {
            if (c0 + cc < p.C) {
                float o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) o[j] = __fdiv_rn(acc[cc][j], ps[j]);
                Pack<T, V>::store_f32(a.out + (long)(c0 + cc) * area + px, o);
            }
        }
    }
}

// One axis of the window grid: ascending origins, the first 0, the last L - win, consecutive gaps <= win.
bool axis_ok(const char *what, const char *axis, const int32_t *o, int n, int L, int win) {
    if (o[0] != 0) { set_error("%s: the first origin of %s is %d, not 0", what, axis, o[0]); return false; }
    for (int i = 1; i < n; ++i) {
        if (o[i] <= o[i - 1]) { set_error("%s: the origins of %s are not ascending (%d after %d)", what, axis, o[i], o[i - 1]); return false; }
        if (o[i] - o[i - 1] > win) {
            set_error("%s: a gap in %s: origins %d and %d are more than the window (%d) apart", what, axis, o[i - 1], o[i], win);
            return false;
        }
    }
    if (o[n - 1] != L - win) { set_error("%s: the last origin of %s is %d, not %d (canvas %d - window %d)", what, axis, o[n - 1], L - win, L, win); return false; }
    return true;
}

// Everything the two entry points share: fills `p`, or sets the error and returns PWW_EINVAL.
int plan_check(const char *what, Plan &p, const int32_t *ys, int ny, const int32_t *xs, int nx, int C, int Hc, int Wc, int h, int w) {
    if (!ys || !xs) { set_error("%s: the window origins ys and xs are required (null pointer)", what); return PWW_EINVAL; }
    if (ny < 1 || nx < 1 || ny > PWW_CANVAS_MAX_WINDOWS || nx > PWW_CANVAS_MAX_WINDOWS || ny * nx > PWW_CANVAS_MAX_WINDOWS) {
        set_error("%s: %d x %d windows (1 .. %d in all)", what, ny, nx, PWW_CANVAS_MAX_WINDOWS);
        return PWW_EINVAL;
    }
    if (h < PWW_CANVAS_MIN_WINDOW || h > PWW_CANVAS_MAX_WINDOW || w < PWW_CANVAS_MIN_WINDOW || w > PWW_CANVAS_MAX_WINDOW) {
        set_error("%s: window %d x %d latent pixels (%d .. %d each)", what, h, w, PWW_CANVAS_MIN_WINDOW, PWW_CANVAS_MAX_WINDOW);
        return PWW_EINVAL;
    }
    if (Hc < h || Wc < w) { set_error("%s: canvas %d x %d is smaller than the window %d x %d", what, Hc, Wc, h, w); return PWW_EINVAL; }
    if (C < 1 || C > PWW_CANVAS_MAX_CHANNELS) { set_error("%s: %d channels (1 .. %d)", what, C, PWW_CANVAS_MAX_CHANNELS); return PWW_EINVAL; }
    if (!axis_ok(what, "ys", ys, ny, Hc, h) || !axis_ok(what, "xs", xs, nx, Wc, w)) return PWW_EINVAL;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < ny; ++i) p.ys[i] = ys[i];
    for (int i = 0; i < nx; ++i) p.xs[i] = xs[i];
    p.ny = ny; p.nx = nx; p.C = C; p.Hc = Hc; p.Wc = Wc; p.h = h; p.w = w;
    return PWW_OK;
}

bool dtype_ok(const char *what, int dtype) {
    if (dtype == PWW_DTYPE_F16 || dtype == PWW_DTYPE_BF16) return true;
    set_error("%s: dtype %d unsupported", what, dtype);
    return false;
}

template <typename T>
int gather_launch(const GatherArgs &a, hipStream_t stream) {
    const Plan &p = a.p;
    const bool wide = p.w % 8 == 0 && aligned16(a.out);
    const long per = (long)p.C * p.h * p.w, lanes = wide ? per / 8 : per;
    const dim3 grid((unsigned)((lanes + CV_GATHER_THREADS - 1) / CV_GATHER_THREADS), (unsigned)(p.ny * p.nx)), block(CV_GATHER_THREADS);
    if (wide) hipLaunchKernelGGL((canvas_gather_kernel<T, 8>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((canvas_gather_kernel<T, 1>), grid, block, 0, stream, a);
    return check_hip(hipGetLastError(), "canvas_gather_kernel launch");
}

template <typename T>
int combine_launch(const CombineArgs &a, hipStream_t stream) {
    const Plan &p = a.p;
    bool wide = p.w % 8 == 0 && p.Wc % 8 == 0 && aligned16(a.eps) && aligned16(a.out) && (a.K == 0 || aligned16(a.masks));
    for (int i = 0; i < p.nx; ++i) wide = wide && p.xs[i] % 8 == 0;
    const long area = (long)p.Hc * p.Wc, lanes = wide ? area / 8 : area;
    const dim3 grid((unsigned)((lanes + CV_COMBINE_THREADS - 1) / CV_COMBINE_THREADS)), block(CV_COMBINE_THREADS);
    if (wide) hipLaunchKernelGGL((canvas_combine_kernel<T, 8>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((canvas_combine_kernel<T, 1>), grid, block, 0, stream, a);
    return check_hip(hipGetLastError(), "canvas_combine_kernel launch");
}

}  // namespace

int canvas_gather(const float *canvas, void *out, const int32_t *ys, int ny, const int32_t *xs, int nx, int C, int Hc, int Wc, int h, int w,
                  float denom, int copies, int dtype, hipStream_t stream) {
    const char *what = "canvas_gather";
    if (!canvas || !out) { set_error("%s: canvas and out are required (null pointer)", what); return PWW_EINVAL; }
    GatherArgs a;
    if (int rc = plan_check(what, a.p, ys, ny, xs, nx, C, Hc, Wc, h, w)) return rc;
    if (copies < 1 || copies > PWW_REGIONS_MAX + 2) { set_error("%s: %d copies (1 .. %d)", what, copies, PWW_REGIONS_MAX + 2); return PWW_EINVAL; }
    if (!(denom > 0.f) || isinf(denom)) { set_error("%s: denom %g is not a finite positive number", what, (double)denom); return PWW_EINVAL; }
    if (!dtype_ok(what, dtype)) return PWW_ENOTSUP;
    if (!arch_ok()) return PWW_ENOTSUP;
    a.canvas = canvas; a.out = out; a.denom = denom; a.copies = copies;
    return dtype == PWW_DTYPE_F16 ? gather_launch<f16>(a, stream) : gather_launch<bf16>(a, stream);
}

int canvas_combine(const void *eps, const float *masks, const float *weights, const float *scales, float g, float *out, const int32_t *ys, int ny,
                   const int32_t *xs, int nx, int K, int C, int Hc, int Wc, int h, int w, int ramp, int dtype, hipStream_t stream) {
    const char *what = "canvas_combine";
    if (!eps || !out) { set_error("%s: eps and out are required (null pointer)", what); return PWW_EINVAL; }
    if (K < 0 || K > PWW_REGIONS_MAX) { set_error("%s: %d regions (0 .. %d)", what, K, PWW_REGIONS_MAX); return PWW_EINVAL; }
    if (K > 0 && (!masks || !weights || !scales)) { set_error("%s: masks, weights and scales are required with region prompts (null pointer)", what); return PWW_EINVAL; }
    CombineArgs a;
    if (int rc = plan_check(what, a.p, ys, ny, xs, nx, C, Hc, Wc, h, w)) return rc;
    if (ramp < 0 || ramp > PWW_CANVAS_MAX_RAMP) { set_error("%s: ramp %d (0 .. %d)", what, ramp, PWW_CANVAS_MAX_RAMP); return PWW_EINVAL; }
    if (!dtype_ok(what, dtype)) return PWW_ENOTSUP;
    if (!arch_ok()) return PWW_ENOTSUP;
    a.eps = eps; a.masks = K ? masks : nullptr; a.weights = K ? weights : nullptr; a.scales = K ? scales : nullptr;
    a.out = out; a.g = g; a.K = K; a.ramp = ramp;
    return dtype == PWW_DTYPE_F16 ? combine_launch<f16>(a, stream) : combine_launch<bf16>(a, stream);
}

}  // namespace pww

PWW_CANVAS_API int pww_canvas_version(void) { return PWW_CANVAS_VERSION; }
PWW_CANVAS_API const char *pww_canvas_last_error(void) { return pww::last_error(); }
PWW_CANVAS_API int pww_canvas_gather(const float *canvas, void *out, const int32_t *ys, int32_t ny, const int32_t *xs, int32_t nx, int32_t C, int32_t Hc,
                                     int32_t Wc, int32_t h, int32_t w, float denom, int32_t copies, int32_t dtype, void *stream) {
    return pww::canvas_gather(canvas, out, ys, ny, xs, nx, C, Hc, Wc, h, w, denom, copies, dtype, static_cast<hipStream_t>(stream));
}
PWW_CANVAS_API int pww_canvas_combine(const void *eps, const float *masks, const float *weights, const float *scales, float g, float *out,
                                      const int32_t *ys, int32_t ny, const int32_t *xs, int32_t nx, int32_t K, int32_t C, int32_t Hc, int32_t Wc, int32_t h,
                                      int32_t w, int32_t ramp, int32_t dtype, void *stream) {
    return pww::canvas_combine(eps, masks, weights, scales, g, out, ys, ny, xs, nx, K, C, Hc, Wc, h, w, ramp, dtype, static_cast<hipStream_t>(stream));
}
