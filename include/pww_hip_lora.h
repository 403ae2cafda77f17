/*
 * libpww_hip_lora.so -- unmerged LoRA adapters chosen per batch row: the low-rank update y += s (x A^T) B^T behind a linear layer, in
 * place, one launch for every row, adapter and column segment of the layer's output. A fifth side library beside libpww_hip.so
 * (include/pww_hip.h), built from csrc/pww_lora.hip for gfx950 (MI355X) and loaded by the Python package on the first call that needs it.
 * It shares the PWW_* return codes and dtype selectors of pww_hip.h and nothing else; every symbol carries the prefix pww_lora_.
 *
 * Device pointers are owned by the caller; the function only enqueues on `stream` and is legal under stream capture; no atomics, nothing
 * waits for another workgroup, plain vector stores, results are bitwise repeatable. Arguments are validated in front of the first HIP
 * runtime call. pww_lora_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_LORA_H
#define PWW_HIP_LORA_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_LORA_VERSION 100   /* major * 100 + minor of THIS library's ABI; pww_lora_desc_t also carries its own size */
#define PWW_LORA_MAX_ADAPTERS 8
#define PWW_LORA_MAX_RANK 128
#define PWW_LORA_MAX_SEGMENTS 3

int pww_lora_version(void);
const char *pww_lora_last_error(void);

/*
 * For every row r with i = row_adapter[r] in [0, n_adapters) and s = row_scale[r] != 0, every token m < T and every column n of segment g
 * (T = the storage type):
 *   t[m][j] = T(sum_k x[r][m][k] * a[i][g][j][k])         fp32 accumulation, rounded once: it is the second product's MFMA operand
 *   u[m][n] = sum_j t[m][j] * b[i][g][n][j]                fp32
 *   y[r][m][g * N / n_seg + n] = T(float(y[...]) + s * u[m][n])                                           one rounding, in place
 * Rows with i < 0 (or i >= n_adapters) or s == 0 keep y bit for bit: their workgroups return before they load any of x, a, b or y.
 *   x            [R][T][K]   with row and token strides;           y [R][T][N] with row and token strides (a view of a wider buffer is fine)
 *   a            [n_adapters][n_seg][rank][K]   contiguous         b [n_adapters][n_seg][N / n_seg][rank]   contiguous
 *   row_adapter  int32 [R], row_scale float [R]                    device memory, read by the kernel: new values need no new capture
 * n_seg > 1: the output is n_seg equal column segments, each with its own factors (the fused q|k|v and k|v projections).
 * rank is the padded rank: an adapter of lower rank is padded with zero rows of a and zero columns of b, which is exact.
 * PWW_EINVAL:  a null pointer, a descriptor shorter than this struct, R / T / K / N < 1, n_seg outside 1 .. 3, n_adapters outside 1 .. 8.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, rank not 32 / 64 / 96 / 128, K no multiple of 32, N no multiple of n_seg or N / n_seg no
 *              multiple of 16, a stride that is no multiple of 8 elements or does not cover its extent, a pointer (x, a, b, y) that is not
 *              16-byte aligned, a tensor of 2^31 elements or more, a device other than gfx950.
 * T is ragged: token rows past T are never read or written.
 */
typedef struct pww_lora_desc {
    uint32_t size;          /* sizeof(pww_lora_desc_t) */
    int32_t dtype;          /* PWW_DTYPE_* */
    int32_t R, T, K, N;     /* rows, tokens per row, in-features, out-features (all segments) */
    int32_t n_seg;          /* 1 .. 3 */
    int32_t rank;           /* 32 | 64 | 96 | 128 */
    int32_t n_adapters;     /* 1 .. 8 */
    int32_t _pad;
    int64_t x_row_stride, x_tok_stride, y_row_stride, y_tok_stride;     /* in elements */
} pww_lora_desc_t;
int pww_lora_fwd(const void *x, const void *a, const void *b, const int32_t *row_adapter, const float *row_scale, void *y,
                 const pww_lora_desc_t *desc, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_LORA_H */
