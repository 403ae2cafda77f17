/*
 * libpww_hip_text.so -- the three pieces of a CLIP text encoder that no other kernel of this project covers: the embedding gather with layer
 * 0's first LayerNorm, the causal self-attention of at most 128 tokens with head dim 64, and the MLP's activation. A side library beside
 * libpww_hip.so (include/pww_hip.h), built from csrc/pww_text.hip for gfx950 (MI355X) and loaded by the Python package on the first call that
 * needs it (pww_hip/text_encode.py). It shares the PWW_* return codes and dtype selectors of pww_hip.h and nothing else; every symbol carries
 * the prefix pww_text_. The GEMMs of the encoder are not here: they run on libpww_hip_linear.so or on the stock GEMM.
 *
 * Device pointers are owned by the caller; the functions only enqueue on `stream` and are legal under stream capture; no atomics, nothing
 * waits for another workgroup, vector stores only, results are bitwise repeatable. Arguments are validated in front of the first HIP runtime
 * call. pww_text_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_TEXT_H
#define PWW_HIP_TEXT_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_TEXT_VERSION 100        /* major * 100 + minor of THIS library's ABI */
#define PWW_TEXT_HEAD_DIM 64        /* the one head dim pww_text_attn_fwd is built for (SD1.x and SD2.x text models) */
#define PWW_TEXT_MAX_TOKENS 128     /* L of pww_text_attn_fwd */
#define PWW_TEXT_MAX_WIDTH 4096     /* C of pww_text_embed_ln */
#define PWW_TEXT_ACT_QUICK_GELU 0   /* x * sigmoid(1.702 x) */
#define PWW_TEXT_ACT_GELU 1         /* 0.5 x (1 + erf(x / sqrt 2)): the form of pww_geglu */

int pww_text_version(void);
const char *pww_text_last_error(void);

/*
 * Embedding gather + layer 0's layer_norm1, one launch:
 *   x[r L + l][:] = T(tok[ids[r][l]][:] + pos[l][:])              h[r L + l][:] = T(LayerNorm(x[r L + l]) * gamma + beta)
 * ids [R][L] int32 (device); tok [V][C], pos [P][C], gamma, beta [C] and the dense outputs x, h [R L][C] in the storage type T. The sum is
 * rounded to T as the stock add of two T tensors rounds it; the statistics of the LayerNorm are those of the ROUNDED x, in fp32 (mean, then
 * the mean of the squared deviations), and h is rounded once. The caller guarantees 0 <= id < V; the kernel clamps an id into the table, so a
 * bad id reads a wrong row and never memory outside the table.
 * PWW_EINVAL:  a null pointer, R / L / V / P < 1.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, C no multiple of 64 or above PWW_TEXT_MAX_WIDTH, L > P, eps <= 0, a pointer that is not 16-byte
 *              aligned, R L C of 2^31 or more, a device other than gfx950.
 */
int pww_text_embed_ln(const void *ids, const void *tok, const void *pos, const void *gamma, const void *beta, void *x, void *h, int32_t R, int32_t L,
                      int32_t C, int32_t V, int32_t P, float eps, int32_t dtype, void *stream);

/*
 * Causal self-attention over a packed projection, head dim 64:
 *   o[r L + i][64 h + :] = sum_{j <= i} T(softmax_j(q_i . k_j / 8)) v_j[:]
 * qkv [R L][3 C] with row stride qkv_stride (elements), C = 64 H: q, k and v of head h at columns 64 h, C + 64 h and 2 C + 64 h. o [R L][C] with
 * row stride o_stride: the heads merged, as out_proj reads them. The scores and the softmax (row maximum subtracted) are fp32; the NORMALISED
 * probabilities are rounded to T once, as the operand of the second product, which accumulates in fp32 and is rounded once. Key j contributes
 * to query i only for j <= i; no row at or past R L is read.
 * PWW_EINVAL:  a null pointer, R / H / L < 1.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, L > PWW_TEXT_MAX_TOKENS, qkv_stride < 3 C or o_stride < C or either no multiple of 8 elements, a
 *              pointer that is not 16-byte aligned, R H > 65535, an extent of 2^31 elements or more, a device other than gfx950.
 */
int pww_text_attn_fwd(const void *qkv, void *o, int32_t R, int32_t H, int32_t L, int64_t qkv_stride, int64_t o_stride, int32_t dtype, void *stream);

/*
 * The MLP's activation, in place over x [M][N] with row stride `stride` (elements); columns at and past N are not touched. Evaluated in fp32
 * and rounded once. Finite for every finite x of the storage type: the sigmoid saturates to 0 and 1.
 * PWW_EINVAL:  a null pointer, M / N < 1.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, an `act` other than PWW_TEXT_ACT_*, N or stride no multiple of 8 elements, stride < N, a pointer
 *              that is not 16-byte aligned, an extent of 2^31 elements or more, a device other than gfx950.
 */
int pww_text_act(void *x, int64_t M, int32_t N, int64_t stride, int32_t act, int32_t dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_TEXT_H */
