// One sampler step as one elementwise launch (include/pww_hip_step.h): the guidance combine, the conversion of the model's prediction, the
// scheduler's affine update, the history write and the next UNet input.
//
//   step_kernel<V, S, O>     flat over the n elements of the latent. A lane owns V consecutive elements: V = 4 with 16-byte fp32 and 8-byte
//                            half accesses, or, where n or an address does not allow that, V = 1. S is the model output's type (f16 / bf16: a
//                            cond / uncond pair combined here; float: one tensor), O the type of the next UNet input. The terms c * h and
//                            e * z are skipped, loads included, when their coefficient is 0 -- uniform branches on kernel arguments.
//
// The arithmetic is fp32, one IEEE operation per step in the order include/pww_hip_step.h writes down; the unit is compiled with
// -ffp-contract=off (build.py PER_FILE_FLAGS) and spells the operations as __f*_rn besides, so a CPU restatement matches bit for bit.
// No atomics, no LDS: plain vector loads and stores.
//
// Built as a library of its own (libpww_hip_step.so): the unit is self-contained, its host plumbing is pww_side_host.h, and only the
// pww_step_* entry points are visible (compiled with -fvisibility=hidden).
#include <math.h>
#define PWW_SIDE_LIB "libpww_hip_step"
#include "pww_side_host.h"
#include "../../include/pww_hip_step.h"

#define PWW_STEP_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

constexpr int ST_THREADS = 64;       // small workgroups: a 4 x 64 x 64 latent is 4096 lanes of 4 elements, spread over 64 CUs

struct StepArgs {
    float *x, *h;
    const void *m0, *m1;
    const float *z;
    void *u;
    float p, r, a, b, c, e, d, g;
    long n;                          // elements of x; the replicas of u lie n elements apart
    int copies;
};

// V consecutive elements of type T <-> fp32 registers: one access of V * sizeof(T) bytes
template <typename T, int V> struct El {
    static __device__ __forceinline__ void load(const T *p, float (&v)[V]) {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (float)p[j];
    }
    static __device__ __forceinline__ void store(T *p, const float (&v)[V]) {
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] = (T)v[j];
    }
};
template <> struct El<float, 4> {
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
template <typename T> struct Half4 {
    typedef typename Vec<T>::v4 v4;
    static __device__ __forceinline__ void load(const T *p, float (&v)[4]) {
        const v4 q = *reinterpret_cast<const v4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)q[j];
    }
    static __device__ __forceinline__ void store(T *p, const float (&v)[4]) {
        const v4 q = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};       // (round to nearest even, once)
        *reinterpret_cast<v4 *>(p) = q;
    }
};
template <> struct El<f16, 4> : Half4<f16> {};
template <> struct El<bf16, 4> : Half4<bf16> {};

template <int V, typename S, typename O>
__global__ void __launch_bounds__(ST_THREADS) step_kernel(const StepArgs a) {
    const long i0 = ((long)blockIdx.x * ST_THREADS + threadIdx.x) * V;
    if (i0 >= a.n) return;           // (V = 4 only when n is a multiple of 4: a lane's elements are all inside)
    float x[V], m[V], q[V];
    El<float, V>::load(a.x + i0, x);
    El<S, V>::load(static_cast<const S *>(a.m0) + i0, m);
    if constexpr (sizeof(S) == 2) {  // the cond / uncond pair: m = u + g (c - u)
        float un[V];
        El<S, V>::load(static_cast<const S *>(a.m1) + i0, un);
#pragma unroll
        for (int j = 0; j < V; ++j) m[j] = __fadd_rn(un[j], __fmul_rn(a.g, __fsub_rn(m[j], un[j])));
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        q[j] = __fadd_rn(__fmul_rn(a.p, x[j]), __fmul_rn(a.r, m[j]));
        x[j] = __fadd_rn(__fmul_rn(a.a, x[j]), __fmul_rn(a.b, q[j]));
    }
    if (a.c != 0.f) {
        float h[V];
        El<float, V>::load(a.h + i0, h);
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = __fadd_rn(x[j], __fmul_rn(a.c, h[j]));
    }
    if (a.e != 0.f) {
        float z[V];
        El<float, V>::load(a.z + i0, z);
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = __fadd_rn(x[j], __fmul_rn(a.e, z[j]));
    }
    El<float, V>::store(a.x + i0, x);
    if (a.h) El<float, V>::store(a.h + i0, q);
    if (a.u) {
        float u[V];
#pragma unroll
        for (int j = 0; j < V; ++j) u[j] = __fdiv_rn(x[j], a.d);
        O *out = static_cast<O *>(a.u) + i0;
        for (int k = 0; k < a.copies; ++k) El<O, V>::store(out + (long)k * a.n, u);
    }
}

template <int V, typename S>
void launch_out(const StepArgs &a, int out, dim3 grid, hipStream_t stream) {
    if (out == PWW_DTYPE_BF16) hipLaunchKernelGGL((step_kernel<V, S, bf16>), grid, dim3(ST_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((step_kernel<V, S, f16>), grid, dim3(ST_THREADS), 0, stream, a);      // (also when there is no u: the type is not used)
}

template <int V>
void launch_src(const StepArgs &a, int src, int out, dim3 grid, hipStream_t stream) {
    if (src == PWW_DTYPE_F16) launch_out<V, f16>(a, out, grid, stream);
    else if (src == PWW_DTYPE_BF16) launch_out<V, bf16>(a, out, grid, stream);
    else launch_out<V, float>(a, out, grid, stream);
}

bool aligned8(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 7) == 0; }

}  // namespace

int step_fwd(float *x, float *h, const void *m0, const void *m1, float g, const float *z, void *u, const float *row, long n, int copies, int src,
             int out, hipStream_t stream) {
    const char *what = "step_fwd";
    if (!x || !m0 || !row) { set_error("%s: x, m0 and row are required (null pointer)", what); return PWW_EINVAL; }
    if (n <= 0) { set_error("%s: %ld elements", what, n); return PWW_EINVAL; }
    const bool pair = src == PWW_DTYPE_F16 || src == PWW_DTYPE_BF16;
    if (!pair && src != PWW_STEP_SRC_F32) { set_error("%s: model output of unknown type %d (f16 0, bf16 1, fp32 2)", what, src); return PWW_ENOTSUP; }
    if (u && out != PWW_DTYPE_F16 && out != PWW_DTYPE_BF16) { set_error("%s: next input of unknown type %d (f16 0, bf16 1)", what, out); return PWW_ENOTSUP; }
    if (pair && !m1) { set_error("%s: a float16 / bfloat16 model output is a cond / uncond pair: m1 is required (null pointer)", what); return PWW_EINVAL; }
    if (u && copies < 1) { set_error("%s: %d copies of the next input (1 or more)", what, copies); return PWW_EINVAL; }
    for (int k = 0; k < PWW_STEP_ROW; ++k)
        if (!isfinite(row[k])) { set_error("%s: coefficient %d of the row (%g) is not finite", what, k, (double)row[k]); return PWW_EINVAL; }
    if (pair && !isfinite(g)) { set_error("%s: the guidance scale %g is not finite", what, (double)g); return PWW_EINVAL; }
    if (row[4] != 0.f && !h) { set_error("%s: c = %g needs the history h (null pointer)", what, (double)row[4]); return PWW_EINVAL; }
    if (row[5] != 0.f && !z) { set_error("%s: e = %g needs the noise z (null pointer)", what, (double)row[5]); return PWW_EINVAL; }
    if (u && !(row[6] > 0.f)) { set_error("%s: the next input is divided by d' = %g (must be positive)", what, (double)row[6]); return PWW_EINVAL; }
    if (n >= (1L << 36)) { set_error("%s: 2^36 elements or more", what); return PWW_ENOTSUP; }
    if (!arch_ok()) return PWW_ENOTSUP;
    StepArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.h = h; a.m0 = m0; a.m1 = pair ? m1 : nullptr; a.z = row[5] != 0.f ? z : nullptr; a.u = u;
    a.p = row[0]; a.r = row[1]; a.a = row[2]; a.b = row[3]; a.c = row[4]; a.e = row[5]; a.d = row[6]; a.g = g;
    a.n = n; a.copies = u ? copies : 0;
    // the wide form: every pointer that is given aligned for its 4-element access (the replicas of u lie 2 n bytes apart: n % 4 keeps them aligned)
    const bool wide = n % 4 == 0 && aligned16(x) && (!h || aligned16(h)) && (!a.z || aligned16(a.z)) && (!u || aligned8(u)) &&
                      (pair ? aligned8(m0) && aligned8(m1) : aligned16(m0));
    const long lanes = wide ? n / 4 : n;
    const dim3 grid((unsigned)((lanes + ST_THREADS - 1) / ST_THREADS));
    if (wide) launch_src<4>(a, src, out, grid, stream);
    else launch_src<1>(a, src, out, grid, stream);
    return check_hip(hipGetLastError(), "step_kernel launch");
}

}  // namespace pww

PWW_STEP_API int pww_step_version(void) { return PWW_STEP_VERSION; }
PWW_STEP_API const char *pww_step_last_error(void) { return pww::last_error(); }
PWW_STEP_API int pww_step_fwd(float *x, float *h, const void *m0, const void *m1, float g, const float *z, void *u, const float *row, int64_t n,
                              int32_t copies, int32_t src, int32_t out, void *stream) {
    return pww::step_fwd(x, h, m0, m1, g, z, u, row, (long)n, copies, src, out, static_cast<hipStream_t>(stream));
}
