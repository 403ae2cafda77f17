/*
 * libpww_hip_convwide.so -- the 160-wide tile (128 x 160 x 64) of the plain 3 x 3 convolution of pww_hip.h (pww_conv3x3_fwd).
 *
 * A shared object of its own beside libpww_hip.so, built from csrc/pww_convwide.hip for gfx950 (MI355X) and loaded by the Python package
 * on the first convolution: the product library sits under its 6 MiB bar by less than the two code objects of this tile. The unit is
 * csrc/pww_conv.hip itself, compiled for this width alone -- kernel, plan and table are one source, so the two libraries cannot disagree
 * about a shape -- and it takes pww_conv_desc_t, the arguments, the workspace and the rules of pww_conv3x3_fwd. It shares the PWW_* return
 * codes and dtype selectors of pww_hip.h and nothing else; every symbol carries the prefix pww_convwide_.
 *
 * Device pointers are owned by the caller; every function only enqueues on `stream` and is legal under stream capture; no atomics,
 * nothing waits for another workgroup, results are bitwise repeatable (and bitwise those of the 64-wide tile at the same split).
 * pww_convwide_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_CONVWIDE_H
#define PWW_HIP_CONVWIDE_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_CONVWIDE_VERSION 100   /* major * 100 + minor of THIS library's ABI; pww_conv_desc_t carries its own size */

int pww_convwide_version(void);
const char *pww_convwide_last_error(void);

/*
 * pww_convwide_takes            1 when the descriptor's plan is the 160-wide tile (tile_n = 160, an entry of the measured table, or a Cout
 *                               that only 160 divides), else 0: pww_conv3x3_fwd launches every other plan and refuses this one, this
 *                               library the other way round (PWW_ENOTSUP).
 * pww_convwide_workspace_bytes, pww_convwide_fwd    pww_conv3x3_workspace_bytes and pww_conv3x3_fwd for such a descriptor.
 */
int pww_convwide_takes(const pww_conv_desc_t *desc);
size_t pww_convwide_workspace_bytes(const pww_conv_desc_t *desc);
int pww_convwide_fwd(const void *x, const void *w, const void *bias, const void *residual, void *y, const pww_conv_desc_t *desc, void *workspace,
                     size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_CONVWIDE_H */
