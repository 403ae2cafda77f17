// Region strength (include/pww_hip_hold.h): a denoising strength per colour of the colour map for img2img. Three kinds of launch:
//
//   hold_map_kernel          colour map uint8 [H][W][3] + K colours and their strength deltas -> fp32 [h][w], h = H / 8, w = W / 8: the base
//                            strength plus, per colour, the share of the pixel's 8 x 8 block that has the colour times the colour's delta,
//                            clamped to [0, 1]. One latent pixel per lane; once per request.
//   hold_feather_kernel      one 1-D pass of the separable Gaussian over a plane in global memory (along the rows, then along the columns:
//                            two launches); the taps ride in the kernel arguments. Once per request, only with a feather.
//   hold_apply_kernel        the hold of one step, in place: x = (S < theta) ? a x0 + b z : x. A lane owns 4 consecutive pixels (16-byte
//                            loads and stores) or, where hw or an address does not allow that, one; the predicate is formed once per pixel
//                            and reused over the C channels; a lane whose pixels are all released loads S and nothing else.
//
// The arithmetic is fp32, one IEEE operation per step in the order include/pww_hip_hold.h writes down; the unit is compiled with
// -ffp-contract=off (build.py PER_FILE_FLAGS) and spells the operations as __f*_rn besides, so a CPU restatement matches bit for bit.
//
// Built as a library of its own (libpww_hip_hold.so): the unit is self-contained, its host plumbing is pww_side_host.h, and only the
// pww_hold_* entry points are visible (compiled with -fvisibility=hidden).
#include <math.h>
#define PWW_SIDE_LIB "libpww_hip_hold"
#include "pww_side_host.h"
#include "../../include/pww_hip_hold.h"

#define PWW_HOLD_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int HD_MAP_THREADS = 256;
constexpr int HD_FEATHER_THREADS = 256;
constexpr int HD_APPLY_THREADS = 64;       // small workgroups: a 4 x 64 x 64 latent is 1024 lanes of 4 pixels, spread over 16 CUs

struct MapArgs {
    const uint8_t *rgb;
    float *out;
    float s0;
    int W, h, w, K;
    uint8_t colors[PWW_HOLD_MAX_COLORS][4];
    float deltas[PWW_HOLD_MAX_COLORS];
};

struct FeatherArgs {
    const float *in;
    float *out;
    int h, w, radius, columns;             // columns = 1: the pass along the columns (the line is a column of the plane)
    float taps[PWW_HOLD_MAX_RADIUS + 1];   // taps[|x|]
};

struct ApplyArgs {
    float *x;
    const float *x0, *z, *S;
    float theta, a, b;
    int C;
    long hw, pixels;                       // pixels = n * hw
};

__global__ void __launch_bounds__(HD_MAP_THREADS) hold_map_kernel(const MapArgs a) {
    const long p = (long)blockIdx.x * HD_MAP_THREADS + threadIdx.x;
    if (p >= (long)a.h * a.w) return;
    const int i = (int)(p / a.w), j = (int)(p - (long)i * a.w);
    const uint8_t *block = a.rgb + ((long)(8 * i) * a.W + 8 * j) * 3;
    int count[PWW_HOLD_MAX_COLORS];
#pragma unroll
    for (int k = 0; k < PWW_HOLD_MAX_COLORS; ++k) count[k] = 0;
    for (int y = 0; y < 8; ++y) {
        const uint8_t *row = block + (long)y * a.W * 3;
        for (int x = 0; x < 8; ++x) {
            const uint8_t r = row[3 * x], g = row[3 * x + 1], b = row[3 * x + 2];
#pragma unroll
            for (int k = 0; k < PWW_HOLD_MAX_COLORS; ++k)
                if (k < a.K) count[k] += (r == a.colors[k][0] && g == a.colors[k][1] && b == a.colors[k][2]) ? 1 : 0;
        }
    }
    float s = a.s0;
#pragma unroll
    for (int k = 0; k < PWW_HOLD_MAX_COLORS; ++k)
        if (k < a.K) s = __fadd_rn(s, __fmul_rn(__fmul_rn((float)count[k], 0.015625f), a.deltas[k]));
    a.out[p] = fminf(fmaxf(s, 0.f), 1.f);
}

// One 1-D pass at pixel `at` of a line of `len` pixels `step` floats apart: sum_x taps[|x|] * line[at + x] / sum_x taps[|x|] over the x inside
// (pww_regions.hip's feather_tap_sum, on global memory).
__device__ __forceinline__ float feather_tap_sum(const float *line, int at, int len, long step, int radius, const float *taps) {
    float acc = 0.f, norm = 0.f;
    const int lo = at - radius < 0 ? -at : -radius, hi = at + radius >= len ? len - 1 - at : radius;
    for (int x = lo; x <= hi; ++x) {
        const float t = taps[x < 0 ? -x : x];
        acc = __fadd_rn(acc, __fmul_rn(t, line[(long)(at + x) * step]));
        norm = __fadd_rn(norm, t);
    }
    return __fdiv_rn(acc, norm);
}

__global__ void __launch_bounds__(HD_FEATHER_THREADS) hold_feather_kernel(const FeatherArgs a) {
    const long p = (long)blockIdx.x * HD_FEATHER_THREADS + threadIdx.x;
    if (p >= (long)a.h * a.w) return;
    const int i = (int)(p / a.w), j = (int)(p - (long)i * a.w);
    a.out[p] = a.columns ? feather_tap_sum(a.in + j, i, a.h, a.w, a.radius, a.taps) : feather_tap_sum(a.in + (long)i * a.w, j, a.w, 1, a.radius, a.taps);
}

template <int V> struct Px;
template <> struct Px<1> {
    static __device__ __forceinline__ void load(const float *p, float (&v)[1]) { v[0] = p[0]; }
    static __device__ __forceinline__ void store(float *p, const float (&v)[1]) { p[0] = v[0]; }
};
template <> struct Px<4> {
    static __device__ __forceinline__ void load(const float *p, float (&v)[4]) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q[j];
    }
    static __device__ __forceinline__ void store(float *p, const float (&v)[4]) {
        const f32x4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4 *>(p) = q;
    }
};

template <int V>
__global__ void __launch_bounds__(HD_APPLY_THREADS) hold_apply_kernel(const ApplyArgs a) {
    const long p0 = ((long)blockIdx.x * HD_APPLY_THREADS + threadIdx.x) * V;      // over the n * hw pixels of S
    if (p0 >= a.pixels) return;
    // (V = 4 only when hw is a multiple of 4: the lane's pixels stay inside one image)
    const long img = p0 / a.hw, q0 = p0 - img * a.hw;
    float s[V];
    Px<V>::load(a.S + p0, s);
    bool held[V], any = false, all = true;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        held[j] = s[j] < a.theta;
        any = any || held[j];
        all = all && held[j];
    }
    if (!any) return;
    for (int c = 0; c < a.C; ++c) {
        const long at = (img * a.C + c) * a.hw + q0;
        float v0[V], vz[V], v[V];
        Px<V>::load(a.x0 + at, v0);
        Px<V>::load(a.z + at, vz);
        if (!all) Px<V>::load(a.x + at, v);
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (held[j]) v[j] = __fadd_rn(__fmul_rn(a.a, v0[j]), __fmul_rn(a.b, vz[j]));
        Px<V>::store(a.x + at, v);
    }
}

bool sigma_ok(const char *what, float sigma) {
    if (sigma >= 0.f && sigma <= PWW_HOLD_MAX_FEATHER) return true;       // (a NaN fails both comparisons)
    set_error("%s: sigma %g outside 0 .. %g", what, (double)sigma, (double)PWW_HOLD_MAX_FEATHER);
    return false;
}

// taps[0 .. radius] of the feather of `sigma` (checked), formed in double and rounded to fp32; returns the radius.
int fill_taps(float sigma, float *taps) {
    if (!(sigma > 0.f)) { taps[0] = 1.f; return 0; }
    const int radius = (int)ceil(3.0 * (double)sigma);
    for (int x = 0; x <= radius; ++x) taps[x] = (float)exp(-0.5 * ((double)x / (double)sigma) * ((double)x / (double)sigma));
    return radius;
}

}  // namespace

int hold_strength_map(const void *rgb, const uint8_t *colors, const float *deltas, float s0, float *out, int H, int W, int K, hipStream_t stream) {
    const char *what = "hold_strength_map";
    if (!rgb || !colors || !deltas || !out) { set_error("%s: rgb, colors, deltas and out are required (null pointer)", what); return PWW_EINVAL; }
    if (K < 1 || K > PWW_HOLD_MAX_COLORS) { set_error("%s: %d colours (1 .. %d)", what, K, PWW_HOLD_MAX_COLORS); return PWW_EINVAL; }
    if (H < 8 || W < 8) { set_error("%s: colour map %d x %d is smaller than one latent pixel (8 x 8)", what, H, W); return PWW_EINVAL; }
    if (!isfinite(s0)) { set_error("%s: the base strength %g is not finite", what, (double)s0); return PWW_EINVAL; }
    for (int k = 0; k < K; ++k)
        if (!isfinite(deltas[k])) { set_error("%s: the strength delta of colour %d (%g) is not finite", what, k, (double)deltas[k]); return PWW_EINVAL; }
    MapArgs a;
    memset(&a, 0, sizeof(a));
    a.rgb = static_cast<const uint8_t *>(rgb);
    a.out = out; a.s0 = s0; a.W = W; a.h = H / 8; a.w = W / 8; a.K = K;
    const long pixels = (long)a.h * a.w;
    if (pixels >= (1L << 31)) { set_error("%s: %d x %d latent pixels: 2^31 or more", what, a.h, a.w); return PWW_ENOTSUP; }
    for (int k = 0; k < K; ++k) {
        for (int ch = 0; ch < 3; ++ch) a.colors[k][ch] = colors[3 * k + ch];
        a.deltas[k] = deltas[k];
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    hipLaunchKernelGGL(hold_map_kernel, dim3((unsigned)((pixels + HD_MAP_THREADS - 1) / HD_MAP_THREADS)), dim3(HD_MAP_THREADS), 0, stream, a);
    return check_hip(hipGetLastError(), "hold_map_kernel launch");
}

int hold_feather(const float *in, float *tmp, float *out, int h, int w, float sigma, hipStream_t stream) {
    const char *what = "hold_feather";
    if (!in || !tmp || !out) { set_error("%s: in, tmp and out are required (null pointer)", what); return PWW_EINVAL; }
    if (tmp == in || tmp == out) { set_error("%s: tmp must be a plane of its own (it is %s)", what, tmp == in ? "in" : "out"); return PWW_EINVAL; }
    if (h < 1 || w < 1) { set_error("%s: bad size %d x %d", what, h, w); return PWW_EINVAL; }
    if (!sigma_ok(what, sigma)) return PWW_EINVAL;
    const long pixels = (long)h * w;
    if (pixels >= (1L << 31)) { set_error("%s: %d x %d pixels: 2^31 or more", what, h, w); return PWW_ENOTSUP; }
    FeatherArgs a;
    memset(&a, 0, sizeof(a));
    a.h = h; a.w = w;
    a.radius = fill_taps(sigma, a.taps);
    if (!arch_ok()) return PWW_ENOTSUP;
    const dim3 grid((unsigned)((pixels + HD_FEATHER_THREADS - 1) / HD_FEATHER_THREADS)), block(HD_FEATHER_THREADS);
    a.in = in; a.out = tmp; a.columns = 0;
    hipLaunchKernelGGL(hold_feather_kernel, grid, block, 0, stream, a);
    if (int rc = check_hip(hipGetLastError(), "hold_feather_kernel launch (rows)")) return rc;
    a.in = tmp; a.out = out; a.columns = 1;
    hipLaunchKernelGGL(hold_feather_kernel, grid, block, 0, stream, a);
    return check_hip(hipGetLastError(), "hold_feather_kernel launch (columns)");
}

int hold_apply(float *x, const float *x0, const float *z, const float *S, float theta, float a, float b, int n, int C, long hw, hipStream_t stream) {
    const char *what = "hold_apply";
    if (!x || !x0 || !z || !S) { set_error("%s: x, x0, z and S are required (null pointer)", what); return PWW_EINVAL; }
    if (n < 1 || C < 1 || hw < 1) { set_error("%s: bad size n=%d C=%d hw=%ld", what, n, C, hw); return PWW_EINVAL; }
    if (!isfinite(theta) || !isfinite(a) || !isfinite(b)) {
        set_error("%s: theta %g, a %g and b %g must be finite", what, (double)theta, (double)a, (double)b);
        return PWW_EINVAL;
    }
    if ((double)n * (double)hw >= (double)(1L << 31) || (double)n * C * (double)hw >= (double)(1L << 40)) {
        set_error("%s: x of 2^40 elements or more (or S of 2^31 or more)", what);
        return PWW_ENOTSUP;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    const ApplyArgs args{x, x0, z, S, theta, a, b, C, hw, (long)n * hw};
    const bool wide = hw % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(z) && aligned16(S);
    const long lanes = wide ? args.pixels / 4 : args.pixels;
    const dim3 grid((unsigned)((lanes + HD_APPLY_THREADS - 1) / HD_APPLY_THREADS)), block(HD_APPLY_THREADS);
    if (wide) hipLaunchKernelGGL(hold_apply_kernel<4>, grid, block, 0, stream, args);
    else hipLaunchKernelGGL(hold_apply_kernel<1>, grid, block, 0, stream, args);
    return check_hip(hipGetLastError(), "hold_apply_kernel launch");
}

int hold_taps(float sigma, float *taps, int cap) {
    const char *what = "hold_taps";
    if (!taps) { set_error("%s: taps is required (null pointer)", what); return PWW_EINVAL; }
    if (!sigma_ok(what, sigma)) return PWW_EINVAL;
    const int radius = sigma > 0.f ? (int)ceil(3.0 * (double)sigma) : 0;
    if (cap < radius + 1) { set_error("%s: room for %d taps, sigma %g needs %d", what, cap, (double)sigma, radius + 1); return PWW_EINVAL; }
    float full[PWW_HOLD_MAX_RADIUS + 1];
    fill_taps(sigma, full);
    memcpy(taps, full, sizeof(float) * (radius + 1));
    return radius;
}

int hold_thresholds(int T, float *theta) {
    const char *what = "hold_thresholds";
    if (!theta) { set_error("%s: theta is required (null pointer)", what); return PWW_EINVAL; }
    if (T < 1 || T > PWW_HOLD_MAX_STEPS) { set_error("%s: %d steps (1 .. %d)", what, T, PWW_HOLD_MAX_STEPS); return PWW_EINVAL; }
    for (int g = 0; g <= T; ++g) theta[g] = (float)((double)(T - g) / (double)T);
    return PWW_OK;
}

}  // namespace pww

PWW_HOLD_API int pww_hold_version(void) { return PWW_HOLD_VERSION; }
PWW_HOLD_API const char *pww_hold_last_error(void) { return pww::last_error(); }
PWW_HOLD_API int pww_hold_strength_map(const void *rgb, const uint8_t *colors, const float *deltas, float s0, float *out, int32_t H, int32_t W,
                                       int32_t K, void *stream) {
    return pww::hold_strength_map(rgb, colors, deltas, s0, out, H, W, K, static_cast<hipStream_t>(stream));
}
PWW_HOLD_API int pww_hold_feather(const float *in, float *tmp, float *out, int32_t h, int32_t w, float sigma, void *stream) {
    return pww::hold_feather(in, tmp, out, h, w, sigma, static_cast<hipStream_t>(stream));
}
PWW_HOLD_API int pww_hold_apply(float *x, const float *x0, const float *z, const float *S, float theta, float a, float b, int32_t n, int32_t C,
                                int64_t hw, void *stream) {
    return pww::hold_apply(x, x0, z, S, theta, a, b, n, C, (long)hw, static_cast<hipStream_t>(stream));
}
PWW_HOLD_API int pww_hold_taps(float sigma, float *taps, int32_t cap) { return pww::hold_taps(sigma, taps, cap); }
PWW_HOLD_API int pww_hold_thresholds(int32_t T, float *theta) { return pww::hold_thresholds(T, theta); }
