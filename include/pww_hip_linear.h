/*
 * libpww_hip_linear.so -- linear layers with the post-processing of the GEMM's output in its epilogue: bias, bias + residual, bias + GEGLU
 * (the feed-forward GEMMs of diffusers' BasicTransformerBlock). A fourth shared object beside libpww_hip.so (include/pww_hip.h),
 * libpww_hip_long.so and libpww_hip_scope.so, built from csrc/pww_linear.hip for gfx950 (MI355X) and loaded by the Python package on the
 * first call that needs it: the product library sits 52 KB under its 6 MiB bar and this unit's code objects are 130 KB. It shares the
 * PWW_* return codes and dtype selectors of pww_hip.h and nothing else; every symbol carries the prefix pww_linear_.
 *
 * Device pointers are owned by the caller; every function only enqueues on `stream` and is legal under stream capture; no atomics,
 * nothing waits for another workgroup, results are bitwise repeatable. Arguments are validated in front of the first HIP runtime call.
 * pww_linear_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_LINEAR_H
#define PWW_HIP_LINEAR_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_LINEAR_VERSION 100   /* major * 100 + minor of THIS library's ABI; pww_linear_desc_t also carries its own size */

int pww_linear_version(void);
const char *pww_linear_last_error(void);

/*
 * y = epilogue(x w^T), fp32 accumulation.
 *   x         [M][K] with row stride x_stride;   w [N][K] contiguous (an nn.Linear weight, or a 1 x 1 conv weight), used in place
 *   bias      [N] (every epilogue but NONE);     residual [M][N] with row stride r_stride (BIAS_RESIDUAL; may alias y)
 *   y         [M][N] with row stride y_stride;   BIAS_GEGLU: [M][N / 2]
 * Epilogues. RESIDUAL and GEGLU have the rounding points of the unfused sequence on tensors of the storage type T (the biased GEMM's output,
 * then the add or pww_geglu); BIAS rounds the accumulator and then the sum, one rounding more than a GEMM whose own epilogue adds the bias:
 *   PWW_LINEAR_NONE            T(acc)
 *   PWW_LINEAR_BIAS            T(T(acc) + bias[n])
 *   PWW_LINEAR_BIAS_RESIDUAL   T(residual[m][n] + T(T(acc) + bias[n]))                      `lin(x) + r`
 *   PWW_LINEAR_BIAS_GEGLU      y[m][j] = T(hv * T(gelu(hg))), hv / hg = the BIAS result at columns j / N / 2 + j   (gelu in erf form: pww_geglu)
 * Requirements: K and N multiples of 64 (BIAS_GEGLU: N / 2 a multiple of 64), row strides multiples of 8 elements (0 = dense), every tensor
 * below 2^31 elements; PWW_ENOTSUP otherwise. tile_n / splitk: 0 = the library's choice (64 / 128 output channels per tile; a measured table
 * for the SD1.5 UNet's shapes, else a K split so that the launch about fills the device). With a K split the fp32 partials go to `workspace`
 * (at least pww_linear_workspace_bytes(desc) bytes, 16-byte aligned, contents need not be initialised) and a second launch folds them in
 * split order and applies the epilogue: no atomics, results bitwise repeatable.
 */
#define PWW_LINEAR_NONE 0
#define PWW_LINEAR_BIAS 1
#define PWW_LINEAR_BIAS_RESIDUAL 2
#define PWW_LINEAR_BIAS_GEGLU 3
typedef struct pww_linear_desc {
    uint32_t size;        /* sizeof(pww_linear_desc_t) */
    int32_t dtype;        /* PWW_DTYPE_* */
    int32_t M, N, K;      /* N = rows of w (2 * inner for BIAS_GEGLU) */
    int32_t epilogue;     /* PWW_LINEAR_* */
    int64_t x_stride, y_stride, r_stride;   /* row strides in elements; 0 = dense (K, the output width, the output width) */
    int32_t tile_n, splitk;
} pww_linear_desc_t;
size_t pww_linear_workspace_bytes(const pww_linear_desc_t *desc);
int pww_linear_fwd(const void *x, const void *w, const void *bias, const void *residual, void *y, const pww_linear_desc_t *desc, void *workspace,
                   size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_LINEAR_H */
