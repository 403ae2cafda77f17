// Region prompts (include/pww_hip_regions.h): a full prompt per colour of the colour map, blended per latent pixel where classifier-free
// guidance is combined. Two launches:
//
//   regions_masks_kernel     colour map uint8 [H][W][3] + K colours -> fp32 [K][h][w], h = H / 8, w = W / 8: the share of each 8 x 8 pixel
//                            block that has the colour, optionally feathered by a separable Gaussian. One 1024-thread workgroup per plane;
//                            the plane (at most 96 x 96 fp32 = 36 KB) stays in LDS for the box count and both feather passes. The pass
//                            along the rows keeps its results in registers (at most 9 pixels per thread) across the barrier and writes
//                            them back in place; the pass along the columns stores to global memory.
//   regions_combine_kernel   the UNet's output of one step [(K + 2) n][C][hw], rows [base x n, region 1 x n, ..., uncond x n], -> the noise
//                            prediction fp32 [n][C][hw]. A lane owns 8 consecutive pixels (16-byte loads of the half-precision rows and of
//                            the masks, 16-byte stores) or, where hw or an address does not allow that, one; the K + 1 coefficients of
//                            its pixels are formed once and reused over the C channels.
//
// The arithmetic is fp32, one IEEE operation per step in the order include/pww_hip_regions.h writes down; the unit is compiled with
// -ffp-contract=off (build.py PER_FILE_FLAGS) and spells the operations as __f*_rn besides, so a CPU restatement matches bit for bit.
//
// Built as a library of its own (libpww_hip_regions.so): the unit is self-contained, its host plumbing is pww_side_host.h, and only the
// pww_regions_* entry points are visible (compiled with -fvisibility=hidden).
#include <math.h>
#define PWW_SIDE_LIB "libpww_hip_regions"
#include "pww_side_host.h"
#include "../../include/pww_hip_regions.h"

#define PWW_REGIONS_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int RG_THREADS = 1024;
constexpr int RG_PER = PWW_REGIONS_MAX_PLANE / RG_THREADS;      // pixels of a plane per thread, at most
constexpr int RG_MAX_RADIUS = 24;                               // ceil(3 * PWW_REGIONS_MAX_FEATHER)
static_assert(RG_PER * RG_THREADS == PWW_REGIONS_MAX_PLANE, "the plane is a whole number of pixels per thread");

struct MaskArgs {
    const uint8_t *rgb;
    float *out;
    int H, W, h, w, radius;
    uint8_t colors[PWW_REGIONS_MAX][4];
    float taps[RG_MAX_RADIUS + 1];       // taps[|x|]
};

// One 1-D pass at pixel `at` of a line of `len` pixels `step` floats apart: sum_x taps[|x|] * line[at + x] / sum_x taps[|x|] over the x inside.
__device__ __forceinline__ float feather_tap_sum(const float *line, int at, int len, int step, int radius, const float *taps) {
    float acc = 0.f, norm = 0.f;
    const int lo = at - radius < 0 ? -at : -radius, hi = at + radius >= len ? len - 1 - at : radius;
    for (int x = lo; x <= hi; ++x) {
        const float t = taps[x < 0 ? -x : x];
        acc = __fadd_rn(acc, __fmul_rn(t, line[(at + x) * step]));
        norm = __fadd_rn(norm, t);
    }
    return __fdiv_rn(acc, norm);
}

__global__ void __launch_bounds__(RG_THREADS) regions_masks_kernel(const MaskArgs a) {
    __shared__ float plane[PWW_REGIONS_MAX_PLANE];
    __shared__ float taps[RG_MAX_RADIUS + 1];
    const int tid = threadIdx.x, k = blockIdx.x, n = a.h * a.w;
    const uint8_t cr = a.colors[k][0], cg = a.colors[k][1], cb = a.colors[k][2];
    if (tid <= RG_MAX_RADIUS) taps[tid] = a.taps[tid];
    for (int p = tid; p < n; p += RG_THREADS) {
        const int i = p / a.w, j = p - i * a.w;
        const uint8_t *block = a.rgb + ((long)(8 * i) * a.W + 8 * j) * 3;
        int count = 0;
        for (int y = 0; y < 8; ++y) {
            const uint8_t *row = block + (long)y * a.W * 3;
#pragma unroll
            for (int x = 0; x < 8; ++x) count += (row[3 * x] == cr && row[3 * x + 1] == cg && row[3 * x + 2] == cb) ? 1 : 0;
        }
        plane[p] = __fmul_rn((float)count, 0.015625f);
    }
    __syncthreads();
    float *out = a.out + (long)k * n;
    if (a.radius == 0) {
        for (int p = tid; p < n; p += RG_THREADS) out[p] = plane[p];
        return;
    }
    float kept[RG_PER];
#pragma unroll
    for (int e = 0; e < RG_PER; ++e) {
        const int p = tid + e * RG_THREADS;
        kept[e] = 0.f;
        if (p < n) {
            const int i = p / a.w, j = p - i * a.w;
            kept[e] = feather_tap_sum(plane + i * a.w, j, a.w, 1, a.radius, taps);
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < RG_PER; ++e) {
        const int p = tid + e * RG_THREADS;
        if (p < n) plane[p] = kept[e];
    }
    __syncthreads();
    for (int p = tid; p < n; p += RG_THREADS) {
        const int i = p / a.w, j = p - i * a.w;
        out[p] = feather_tap_sum(plane + j, i, a.h, a.w, a.radius, taps);
    }
}

struct CombineArgs {
    const void *eps;
    const float *masks, *weights, *scales;
    float *out;
    float g;
    int n, K, C;
    long hw;
};

template <typename T, int V> struct Px;
template <typename T> struct Px<T, 1> {
    static __device__ __forceinline__ void load(const T *p, float (&v)[1]) { v[0] = (float)p[0]; }
    static __device__ __forceinline__ void load_f32(const float *p, float (&v)[1]) { v[0] = p[0]; }
    static __device__ __forceinline__ void store(float *p, const float (&v)[1]) { p[0] = v[0]; }
};
template <typename T> struct Px<T, 8> {
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
    static __device__ __forceinline__ void store(float *p, const float (&v)[8]) {
        const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
        *reinterpret_cast<f32x4 *>(p) = lo;
        *reinterpret_cast<f32x4 *>(p + 4) = hi;
    }
};

template <typename T, int V>
__global__ void __launch_bounds__(256) regions_combine_kernel(const CombineArgs a) {
    const int img = blockIdx.y;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (p0 >= a.hw) return;
    // the K + 1 coefficients of this lane's pixels: c[0] = w_0 g, c[k] = w_k s_k
    float c[PWW_REGIONS_MAX + 1][V], sum[V];
#pragma unroll
    for (int k = 0; k < PWW_REGIONS_MAX; ++k) {
        if (k < a.K) {
            const float ak = a.weights[(long)img * a.K + k], sk = a.scales[(long)img * a.K + k];
            float m[V];
            Px<T, V>::load_f32(a.masks + ((long)img * a.K + k) * a.hw + p0, m);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float w = __fmul_rn(ak, m[j]);
                sum[j] = k == 0 ? w : __fadd_rn(sum[j], w);
                c[k + 1][j] = __fmul_rn(w, sk);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) c[0][j] = __fmul_rn(__fsub_rn(1.f, sum[j]), a.g);
    const T *eps = static_cast<const T *>(a.eps);
    const long row = (long)a.C * a.hw;                       // one image of eps
    for (int ch = 0; ch < a.C; ++ch) {
        const long at = ((long)img * a.C + ch) * a.hw + p0;  // this image's channel inside a block of n rows
        float u[V], e[V], acc[V];
        Px<T, V>::load(eps + (long)(a.K + 1) * a.n * row + at, u);
        Px<T, V>::load(eps + at, e);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = __fadd_rn(u[j], __fmul_rn(c[0][j], __fsub_rn(e[j], u[j])));
#pragma unroll
        for (int k = 0; k < PWW_REGIONS_MAX; ++k) {
            if (k < a.K) {
                Px<T, V>::load(eps + (long)(k + 1) * a.n * row + at, e);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(c[k + 1][j], __fsub_rn(e[j], u[j])));
            }
        }
        Px<T, V>::store(a.out + at, acc);
    }
}

bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int combine_launch(const CombineArgs &a, hipStream_t stream) {
    const bool wide = a.hw % 8 == 0 && al16(a.eps) && al16(a.masks) && al16(a.out);
    const long lanes = wide ? a.hw / 8 : a.hw;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)a.n), block(256);
    if (wide) hipLaunchKernelGGL((regions_combine_kernel<T, 8>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((regions_combine_kernel<T, 1>), grid, block, 0, stream, a);
    return check_hip(hipGetLastError(), "regions_combine_kernel launch");
}

}  // namespace

int regions_masks(const void *rgb, int H, int W, const uint8_t *colors, int K, float feather, float *out, hipStream_t stream) {
    if (!rgb || !colors || !out) { set_error("regions_masks: rgb, colors and out are required"); return PWW_EINVAL; }
    if (K < 1 || K > PWW_REGIONS_MAX) { set_error("regions_masks: %d regions (1 .. %d)", K, PWW_REGIONS_MAX); return PWW_EINVAL; }
    if (H < 8 || W < 8) { set_error("regions_masks: colour map %d x %d is smaller than one latent pixel (8 x 8)", H, W); return PWW_EINVAL; }
    if (!(feather >= 0.f) || !(feather <= PWW_REGIONS_MAX_FEATHER)) {
        set_error("regions_masks: feather %g outside 0 .. %g", (double)feather, (double)PWW_REGIONS_MAX_FEATHER);
        return PWW_EINVAL;
    }
    MaskArgs a;
    memset(&a, 0, sizeof(a));
    a.rgb = static_cast<const uint8_t *>(rgb);
    a.out = out;
    a.H = H; a.W = W; a.h = H / 8; a.w = W / 8;
    if ((long)a.h * a.w > PWW_REGIONS_MAX_PLANE) {
        set_error("regions_masks: %d x %d latent pixels exceed the %d of one plane", a.h, a.w, PWW_REGIONS_MAX_PLANE);
        return PWW_ENOTSUP;
    }
    for (int k = 0; k < K; ++k)
        for (int ch = 0; ch < 3; ++ch) a.colors[k][ch] = colors[3 * k + ch];
    a.radius = feather > 0.f ? (int)ceil(3.0 * (double)feather) : 0;
    for (int x = 0; x <= a.radius; ++x) a.taps[x] = (float)exp(-0.5 * ((double)x / (double)feather) * ((double)x / (double)feather));
    if (!arch_ok()) return PWW_ENOTSUP;
    hipLaunchKernelGGL(regions_masks_kernel, dim3(K), dim3(RG_THREADS), 0, stream, a);
    return check_hip(hipGetLastError(), "regions_masks_kernel launch");
}

int regions_combine(const void *eps, const float *masks, const float *weights, const float *scales, float g, float *out, int n, int K, int C,
                    long hw, int dtype, hipStream_t stream) {
    if (!eps || !masks || !weights || !scales || !out) { set_error("regions_combine: eps, masks, weights, scales and out are required"); return PWW_EINVAL; }
    if (K < 1 || K > PWW_REGIONS_MAX) { set_error("regions_combine: %d regions (1 .. %d)", K, PWW_REGIONS_MAX); return PWW_EINVAL; }
    if (n < 1 || n > 65535 || C < 1 || hw < 1) { set_error("regions_combine: bad size n=%d C=%d hw=%ld (n 1 .. 65535)", n, C, hw); return PWW_EINVAL; }
    if (dtype != PWW_DTYPE_F16 && dtype != PWW_DTYPE_BF16) { set_error("regions_combine: dtype %d unsupported", dtype); return PWW_ENOTSUP; }
    if (hw >= (1L << 31) || (double)(K + 2) * n * C * (double)hw >= (double)(1L << 40)) {
        set_error("regions_combine: eps of 2^40 elements or more");
        return PWW_ENOTSUP;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    const CombineArgs a{eps, masks, weights, scales, out, g, n, K, C, hw};
    return dtype == PWW_DTYPE_F16 ? combine_launch<f16>(a, stream) : combine_launch<bf16>(a, stream);
}

}  // namespace pww

PWW_REGIONS_API int pww_regions_version(void) { return PWW_REGIONS_VERSION; }
PWW_REGIONS_API const char *pww_regions_last_error(void) { return pww::last_error(); }
PWW_REGIONS_API int pww_regions_masks(const void *rgb, int32_t H, int32_t W, const uint8_t *colors, int32_t K, float feather, float *out, void *stream) {
    return pww::regions_masks(rgb, H, W, colors, K, feather, out, static_cast<hipStream_t>(stream));
}
PWW_REGIONS_API int pww_regions_combine(const void *eps, const float *masks, const float *weights, const float *scales, float g, float *out,
                                        int32_t n, int32_t K, int32_t C, int64_t hw, int32_t dtype, void *stream) {
    return pww::regions_combine(eps, masks, weights, scales, g, out, n, K, C, (long)hw, dtype, static_cast<hipStream_t>(stream));
}
