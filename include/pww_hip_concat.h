/*
 * libpww_hip_concat.so -- the two readers of `torch.cat([x1, x2], dim=1)` in an up block of the UNet, reading the two halves where they
 * lie, so that the concatenated tensor is never written:
 *
 *     pww_concat_group_norm_fwd    y = act(GroupNorm(cat(x1, x2)) * gamma + beta)          (norm1 of the block's ResnetBlock2D)
 *     pww_concat_convtail_fwd      y = conv3x3(h, w) + conv1x1(cat(x1, x2), wsc) + bias + bias2   (conv2 + the 1 x 1 shortcut)
 *
 * Each is the one-source kernel of libpww_hip.so (pww_group_norm_fwd, channels_last) / libpww_hip_convtail.so (pww_convtail_fwd) with ONE
 * change: a thread (GroupNorm) or a K-slab (shortcut) selects base pointer, row pitch and channel offset of its source once, without a
 * branch. Launch form, slab sizes, tile, K split, summation order and rounding points are those of the one-source entry point for
 * C = C1 + C2 channels, so the result equals, bit for bit, the one-source result on the concatenated tensor.
 *
 * A shared object of its own, built from csrc/pww_concat.hip for gfx950 (MI355X) and loaded by the Python package on the first call that
 * needs it. It shares the PWW_* return codes and selectors of pww_hip.h and nothing else; every symbol carries the prefix pww_concat_.
 *
 * Device pointers are owned by the caller; every function only enqueues on `stream` and is legal under stream capture; no atomics,
 * nothing waits for another workgroup, results are bitwise repeatable. Arguments are validated in front of the first HIP runtime call:
 * PWW_ENOTSUP for a shape the kernels do not take, PWW_EINVAL for a missing or misaligned pointer, a descriptor older than the library
 * or a workspace that is too small. pww_concat_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_CONCAT_H
#define PWW_HIP_CONCAT_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_CONCAT_VERSION 100   /* major * 100 + minor of THIS library's ABI; the descriptors also carry their own size */

int pww_concat_version(void);
const char *pww_concat_last_error(void);

/*
 * GroupNorm over the channels of two channels_last tensors laid end to end, then the affine map and the activation:
 *   x1 [B][HW][C1], x2 [B][HW][C2]  ->  y [B][HW][C1 + C2];   gamma, beta [C1 + C2] or null;   G groups of (C1 + C2) / G channels, which
 *   may straddle the boundary between the two tensors.
 * Requirements (PWW_ENOTSUP otherwise): what pww_group_norm_fwd asks of a channels_last tensor of C1 + C2 channels (HW a multiple of 8,
 * (C1 + C2) % G == 0, G <= 32, C1 + C2 <= 4096), and C1, C2 multiples of 8. Every pointer 16-byte aligned.
 * `workspace`: at least pww_concat_group_norm_workspace_bytes(desc) bytes (0 = unsupported description); contents need not be initialised.
 */
typedef struct pww_concat_gn_desc {
    uint32_t size;        /* sizeof(pww_concat_gn_desc_t) */
    int32_t dtype;        /* PWW_DTYPE_* */
    int32_t B, C1, C2, HW, G;
    float eps;
    int32_t act;          /* PWW_ACT_* */
    int32_t _pad;
} pww_concat_gn_desc_t;
size_t pww_concat_group_norm_workspace_bytes(const pww_concat_gn_desc_t *desc);
int pww_concat_group_norm_fwd(const void *x1, const void *x2, const void *gamma, const void *beta, void *y, const pww_concat_gn_desc_t *desc,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * pww_convtail_fwd (include/pww_hip_convtail.h) with the shortcut's input in two parts:
 *   y[b][oy][ox][n] = T( sum_{ky,kx,ci} x[b][oy+ky-1][ox+kx-1][ci] w[n][ky][kx][ci]
 *                        + sum_{c < C1} x1[b][oy][ox][c] wsc[n][c] + sum_{c < C2} x2[b][oy][ox][c] wsc[n][C1 + c] + bias[n] + bias2[n] )
 *   x [B][H][W][Cin], w [Cout][3][3][Cin], x1 [B][H][W][C1], x2 [B][H][W][C2], wsc [Cout][C1 + C2], bias, bias2 [Cout], y [B][H][W][Cout].
 * Requirements: Cin, C1, C2 and Cout multiples of 64, every tensor below 2^31 elements; PWW_ENOTSUP otherwise. x, w, x1, x2, wsc and y
 * 16-byte aligned, the biases 8-byte aligned; PWW_EINVAL otherwise. tile_n / splitk: 0 = the choice pww_convtail_fwd makes for C2 = C1 + C2.
 * With a K split the fp32 partials go to `workspace` (pww_concat_convtail_workspace_bytes(desc) bytes, 16-byte aligned).
 */
typedef struct pww_concat_tail_desc {
    uint32_t size;        /* sizeof(pww_concat_tail_desc_t) */
    int32_t dtype;        /* PWW_DTYPE_* */
    int32_t B, H, W;
    int32_t Cin, C1, C2, Cout;
    int32_t tile_n, splitk;
    int32_t _pad;
} pww_concat_tail_desc_t;
size_t pww_concat_convtail_workspace_bytes(const pww_concat_tail_desc_t *desc);
int pww_concat_convtail_fwd(const void *x, const void *w, const void *x1, const void *x2, const void *wsc, const void *bias, const void *bias2, void *y,
                            const pww_concat_tail_desc_t *desc, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_CONCAT_H */
