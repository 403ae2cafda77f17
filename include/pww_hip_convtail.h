/*
 * libpww_hip_convtail.so -- the second 3 x 3 convolution of a ResnetBlock2D that changes its channel count, with the block's 1 x 1
 * shortcut convolution as further K-slabs of the same implicit GEMM:
 *
 *     y = conv3x3(x, w) + conv1x1(x2, w2) + bias + bias2
 *
 * A shared object of its own beside libpww_hip.so (include/pww_hip.h), built from csrc/pww_conv_tail.hip for gfx950 (MI355X) and loaded by
 * the Python package on the first call that needs it: the product library sits under its 6 MiB bar by less than this unit's code objects,
 * and the convolution's code objects in it stay as they are. It shares the PWW_* return codes and dtype selectors of pww_hip.h and nothing
 * else; every symbol carries the prefix pww_convtail_.
 *
 * Device pointers are owned by the caller; every function only enqueues on `stream` and is legal under stream capture; no atomics,
 * nothing waits for another workgroup, results are bitwise repeatable. Arguments are validated in front of the first HIP runtime call.
 * pww_convtail_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_CONVTAIL_H
#define PWW_HIP_CONVTAIL_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_CONVTAIL_VERSION 100   /* major * 100 + minor of THIS library's ABI; pww_convtail_desc_t also carries its own size */

int pww_convtail_version(void);
const char *pww_convtail_last_error(void);

/*
 * y[b][oy][ox][n] = T( sum_{ky,kx,ci} x[b][oy+ky-1][ox+kx-1][ci] w[n][ky][kx][ci]  +  sum_c x2[b][oy][ox][c] w2[n][c]  +  bias[n] + bias2[n] )
 * with fp32 accumulation and ONE rounding to the storage type T (the unfused sequence -- 1 x 1 convolution, 3 x 3 convolution, bias,
 * residual add on T tensors -- rounds the shortcut, the convolution, the biased convolution and the sum).
 *   x      [B][H][W][Cin]  (channels_last), zero padding 1, stride 1      w   [Cout][3][3][Cin]  (a channels_last nn.Conv2d weight)
 *   x2     [B][H][W][C2]   (channels_last), the same B, H, W              w2  [Cout][C2]         (a 1 x 1 nn.Conv2d weight, used in place)
 *   bias, bias2  [Cout], both required                                    y   [B][H][W][Cout]
 * Requirements: Cin and C2 multiples of 64, Cout a multiple of 64 or of 160, every tensor below 2^31 elements; PWW_ENOTSUP otherwise. x, w, x2,
 * w2 and y 16-byte aligned, the biases 8-byte aligned; PWW_EINVAL otherwise.
 * tile_n / splitk: 0 = the library's choice (64 / 128 / 160 output channels per tile, a width that divides Cout; a measured table for the SD1.5 UNet's shapes, else a K split
 * so that the launch about fills the device). K runs over 9 Cin / 64 + C2 / 64 slabs of 64; a split boundary may fall anywhere in them.
 * With a K split the fp32 partials go to `workspace` (at least pww_convtail_workspace_bytes(desc) bytes, 16-byte aligned, contents need not
 * be initialised) and a second launch folds them in split order and applies the epilogue.
 */
typedef struct pww_convtail_desc {
    uint32_t size;        /* sizeof(pww_convtail_desc_t) */
    int32_t dtype;        /* PWW_DTYPE_* */
    int32_t B, H, W;
    int32_t Cin, C2, Cout;
    int32_t tile_n, splitk;
} pww_convtail_desc_t;
size_t pww_convtail_workspace_bytes(const pww_convtail_desc_t *desc);
int pww_convtail_fwd(const void *x, const void *w, const void *x2, const void *w2, const void *bias, const void *bias2, void *y,
                     const pww_convtail_desc_t *desc, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_CONVTAIL_H */
