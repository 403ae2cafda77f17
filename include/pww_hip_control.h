/*
 * libpww_hip_control.so -- the residuals of a ControlNet in one launch: its 1 x 1 "zero convolutions" (thirteen for the SD1.5 topology), the
 * scaling by the conditioning scale and the add into the UNet's skip tensors and mid-block output as ONE grouped GEMM. A side library beside
 * libpww_hip.so (include/pww_hip.h), built from csrc/pww_control.hip for gfx950 (MI355X) and loaded by the Python package on the first call
 * that needs it. It shares the PWW_* return codes and dtype selectors of pww_hip.h and nothing else; every symbol carries the prefix
 * pww_control_.
 *
 * Device pointers are owned by the caller; pww_control_fwd only enqueues ONE kernel on `stream` and is legal under stream capture: no split-K,
 * no workspace, no atomics, nothing waits for another workgroup, results are bitwise repeatable. Arguments are validated in front of the
 * first HIP runtime call. pww_control_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_CONTROL_H
#define PWW_HIP_CONTROL_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_CONTROL_VERSION 100   /* major * 100 + minor of THIS library's ABI; pww_control_desc_t also carries its own size */
#define PWW_CONTROL_MAX_PROBLEMS 16
#define PWW_CONTROL_TILE_M 128
#define PWW_CONTROL_TILE_N 64

int pww_control_version(void);
const char *pww_control_last_error(void);

/*
 * For each problem p < n, fp32 accumulation, T = the storage type:
 *   out_p[m][c] = T(skip_p[m][c] + s * (sum_k h_p[m][k] * w_p[c][k] + bias_p[c]))        skip_p given
 *   out_p[m][c] = T(s * (sum_k h_p[m][k] * w_p[c][k] + bias_p[c]))                       skip_p NULL
 *   s = scale_dev[scale_index], an fp32 word in device memory that the KERNEL reads: it is not a kernel argument, so a launch captured into a
 *   graph follows the word as it is at each replay.
 * Rounding: ONE rounding, at the store. The stock sequence (a 1 x 1 convolution, a multiplication by the scale, an add into the skip, each
 * on tensors of type T) rounds three times, so this result is the more accurate one and differs from the stock one within those roundings.
 * s == 0 is exact: out_p = skip_p bit for bit (zeros without a skip), whatever h holds -- the ControlNet outside its guidance window.
 *
 *   h      [M][K] with row stride h_stride (the [B H W, C] view of a channels_last hidden state)
 *   w      [N][K] dense: a 1 x 1 convolution's weight, used in place
 *   bias   [N]
 *   skip   [M][N] with row stride skip_stride, or NULL;   out [M][N] with row stride out_stride; out may alias skip (same pointer and stride)
 * Requirements: 1 <= n <= 16; K and N multiples of 64; row strides multiples of 8 elements that cover their rows (0 = dense); any M >= 1 (the
 * M tail loads clamped rows and masks its store); h, w, skip, out 16-byte aligned, bias 8-byte aligned; every tensor below 2^31 elements.
 * PWW_EINVAL for a missing pointer, a descriptor of another size or a count outside 1 .. 16, PWW_ENOTSUP for the rest.
 *
 * The launch: one workgroup per 128 (M) x 64 (N) output tile of any problem. The problem table travels by value in the kernel arguments; a
 * workgroup finds its (problem, tile) from the prefix sums of the problems' tile counts. Tiles are issued problem by problem in descending K
 * (ties: in the caller's order), so the tiles with the longest K loop start first and do not form the launch's tail.
 */
typedef struct pww_control_problem {
    const void *h, *w, *bias, *skip;
    void *out;
    int32_t M, N, K;
    int32_t _pad;
    int64_t h_stride, skip_stride, out_stride;   /* row strides in elements; 0 = dense (K, N, N) */
} pww_control_problem_t;
typedef struct pww_control_desc {
    uint32_t size;        /* sizeof(pww_control_desc_t) */
    int32_t dtype;        /* PWW_DTYPE_* */
    int32_t n;            /* problems */
    int32_t scale_index;  /* which word of scale_dev, >= 0 */
} pww_control_desc_t;
int pww_control_fwd(const pww_control_problem_t *problems, const pww_control_desc_t *desc, const float *scale_dev, void *stream);

/*
 * Host only, no HIP call: the tile list the launch of these problems walks, in workgroup order. Writes (problem index in the caller's order,
 * m0, n0) for the first min(tiles, cap) tiles to out_tiles ([cap][3]; may be NULL with cap 0) and returns the number of tiles, or a negative
 * PWW_* code for a table pww_control_fwd refuses. Only M, N, K and the strides of the problems are read.
 */
int pww_control_plan(const pww_control_problem_t *problems, int32_t n, int32_t *out_tiles, int32_t cap);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_CONTROL_H */
