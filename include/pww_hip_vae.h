/*
 * libpww_hip_vae.so -- the two pieces of the AutoencoderKL decoder that no other kernel of this project covers: the mid block's one-head
 * attention with head dim 512, and the decoder's tail (conv_norm_out -> SiLU -> conv_out to 3 channels -> image). A side library beside
 * libpww_hip.so (include/pww_hip.h), built from csrc/pww_vae.hip for gfx950 (MI355X) and loaded by the Python package on the first call that
 * needs it (pww_hip/vae.py). It shares the PWW_* return codes and dtype selectors of pww_hip.h and nothing else; every symbol carries the
 * prefix pww_vae_.
 *
 * Device pointers are owned by the caller; the functions only enqueue on `stream` and are legal under stream capture; no atomics, nothing
 * waits for another workgroup, vector stores only, results are bitwise repeatable. Arguments are validated in front of the first HIP runtime
 * call. pww_vae_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_VAE_H
#define PWW_HIP_VAE_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_VAE_VERSION 100     /* major * 100 + minor of THIS library's ABI; the descriptors also carry their own size */
#define PWW_VAE_HEAD_DIM 512    /* the one head dim pww_vae_attn_fwd is built for */
#define PWW_VAE_TAIL_CHANNELS 128
#define PWW_VAE_TAIL_GROUPS 32
#define PWW_VAE_TAIL_MAX_CHUNKS 64
#define PWW_VAE_OUT_SAMPLE 0    /* [B][3][H][W] in the storage type */
#define PWW_VAE_OUT_UINT8 1     /* [B][H][W][3] uint8 */

int pww_vae_version(void);
const char *pww_vae_last_error(void);

/*
 * One-head attention, head dim 512, flash-style: the N x N scores are never stored.
 *   o[b][n][:] = sum_m softmax_m(scale * q[b][n] . k[b][m]) v[b][m][:]          scale = 1 / sqrt(512) unless desc->scale > 0
 * q, k, v: rows of 512 elements with a row stride and a batch stride each (in elements), so the three slices of one [B][N][1536] GEMM output
 * are read where they lie; o: [B][N][512] rows with its own strides -- the channels_last [B][512][H][W] tensor itself. The scores and the
 * softmax are fp32; the probabilities are rounded to the storage type once, as the operand of the second product; the row sum is that of
 * the unrounded probabilities. Any N >= 1 (ragged last query block and last key block), any B >= 1.
 * PWW_EINVAL:  a null pointer, a descriptor shorter than this struct, B < 1 or N < 1.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, D != 512, a stride that is no multiple of 8 elements or a row stride below 512, a pointer that
 *              is not 16-byte aligned, an extent of 2^31 elements or more, more than 65535 images, a device other than gfx950.
 */
typedef struct pww_vae_attn_desc {
    uint32_t size;          /* sizeof(pww_vae_attn_desc_t) */
    int32_t dtype;          /* PWW_DTYPE_* */
    int32_t B, N, D;        /* images, tokens (queries = keys), head dim (512) */
    float scale;            /* <= 0: 1 / sqrt(D) */
    int64_t q_batch_stride, q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride, o_batch_stride, o_row_stride;
} pww_vae_attn_desc_t;
int pww_vae_attn_fwd(const void *q, const void *k, const void *v, void *o, const pww_vae_attn_desc_t *desc, void *stream);

/*
 * The decoder's tail: y = conv3x3(SiLU(GroupNorm_32(x)), w) + bias for a channels_last x [B][128][H][W] (memory [B][H][W][128]), then
 *   PWW_VAE_OUT_SAMPLE   out[b][o][h][w] = T(y)                                                     ([B][3][H][W], the storage type)
 *   PWW_VAE_OUT_UINT8    out[b][h][w][o] = (uint8) rint(255 * min(max(y / 2 + 0.5, 0), 1))          ([B][H][W][3]; rint: half to even)
 * The convolution's zero padding applies to the activation: a tap outside the image contributes 0. From the normalised value to y everything
 * is fp32: nothing in between is rounded to the storage type.
 * Two launches. pww_vae_tail_stats forms, per image, chunk of pixels and group, the fp32 sum and sum of squares of x in a fixed order (and,
 * when `w` is given, the fp32 copy of the weight the second launch reads) in `ws`; the same input gives the same bytes. The second launch
 * adds the chunks up in their order, normalises, and convolves. pww_vae_tail_fwd enqueues both; `ws` needs pww_vae_tail_workspace_bytes.
 *   gamma, beta  [128] (storage type): conv_norm_out's affine           w  [3][128][3][3] contiguous (storage type)       bias  [3]
 * PWW_EINVAL:  a null pointer, a descriptor shorter than this struct, B / H / W < 1, a workspace that is too small.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, C != 128, `out` other than the two forms, eps <= 0, x not 16-byte aligned, a tensor of 2^31
 *              elements or more, more than 65535 images, a device other than gfx950.
 */
typedef struct pww_vae_tail_desc {
    uint32_t size;          /* sizeof(pww_vae_tail_desc_t) */
    int32_t dtype;          /* PWW_DTYPE_* */
    int32_t B, H, W, C;     /* C: 128 */
    int32_t out;            /* PWW_VAE_OUT_* */
    float eps;
} pww_vae_tail_desc_t;
size_t pww_vae_tail_workspace_bytes(const pww_vae_tail_desc_t *desc);
int pww_vae_tail_chunks(const pww_vae_tail_desc_t *desc);      /* chunks per image of the statistics launch (0: unsupported) */
int pww_vae_tail_stats(const void *x, const void *w, const pww_vae_tail_desc_t *desc, void *ws, size_t ws_bytes, void *stream);
int pww_vae_tail_fwd(const void *x, const void *gamma, const void *beta, const void *w, const void *bias, void *out,
                     const pww_vae_tail_desc_t *desc, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_VAE_H */
