/*
 * libpww_hip_step.so -- one sampler step as one elementwise launch: the classifier-free-guidance combine, the conversion of the model's
 * prediction, the scheduler's update, the history write and the next UNet input. Euler, Euler ancestral, DDIM and DPM-Solver++(2M) are the
 * same affine update with different scalars (pww_hip/steps.py builds the seven numbers of a step on the host, in double). A shared object of
 * its own beside libpww_hip.so (include/pww_hip.h) and the other side libraries, built from csrc/pww_step.hip for gfx950 (MI355X) and loaded
 * by the Python package on the first step that takes this route. It shares the PWW_* return codes of pww_hip.h and nothing else; every symbol
 * carries the prefix pww_step_.
 *
 * Device pointers are owned by the caller; the launching function only enqueues on `stream` and is legal under stream capture; no atomics, no
 * LDS, nothing waits for another workgroup, plain vector loads and stores only, results are bitwise repeatable. The unit is compiled without
 * FMA contraction and every operation below is a single IEEE fp32 operation in the order written, so a CPU restatement in fp32 matches bit
 * for bit. Arguments are validated in front of the first HIP runtime call. pww_step_last_error() describes the last failure of the calling
 * thread.
 */
#ifndef PWW_HIP_STEP_H
#define PWW_HIP_STEP_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_STEP_VERSION 100        /* major * 100 + minor of THIS library's ABI */
#define PWW_STEP_SRC_F32 2          /* `src` of a model output that is ONE fp32 tensor; PWW_DTYPE_F16 / PWW_DTYPE_BF16: a cond / uncond pair */
#define PWW_STEP_ROW 7              /* floats of a step's row: p, r, a, b, c, e, d' */

int pww_step_version(void);
const char *pww_step_last_error(void);

/*
 * One step over `n` elements, flat:
 *   x       device, fp32 [n]           the latent, updated IN PLACE
 *   h       device, fp32 [n] or null   the previous step's q; read only if c != 0, then overwritten with this step's q. Null: no history
 *                                      is kept (c must be 0)
 *   m0, m1  device                     the model output. src = PWW_DTYPE_F16 / PWW_DTYPE_BF16: m0 = cond and m1 = uncond, [n] of that type,
 *                                      and m = m1 + g * (m0 - m1) (one subtraction, one multiplication, one addition). src = PWW_STEP_SRC_F32:
 *                                      m0 is m itself, fp32 [n]; m1 and g are ignored
 *   z       device, fp32 [n] or null   unit Gaussian noise; read only if e != 0
 *   u       device, [copies][n] of type `out` (PWW_DTYPE_F16 / PWW_DTYPE_BF16), or null: the next UNet input, `copies` equal replicas
 *   row     HOST, fp32 [PWW_STEP_ROW]  p, r, a, b, c, e, d' (they travel in the kernel arguments)
 * Per element, each line one IEEE fp32 operation per operator, in this order:
 *   q  = (p * x) + (r * m)
 *   x' = (a * x) + (b * q)
 *   x' = x' + (c * h)          only if c != 0
 *   x' = x' + (e * z)          only if e != 0
 *   u  = x' / d'               rounded once (to nearest even) to `out`, the same value into every replica; only if u is not null
 *   x  = x';  h = q            (h only if not null)
 * A term whose coefficient is exactly 0 is absent: its tensor is not read (a NaN there changes nothing) and its pointer may be null.
 * One launch. A lane owns 4 consecutive elements (16-byte fp32, 8-byte half accesses) when n is a multiple of 4 and every pointer given is
 * aligned for that form, else one element.
 * PWW_EINVAL: x, m0 or row null; m1 null with a half `src`; h null with c != 0; z null with e != 0; n <= 0; copies < 1 with u given; a
 * coefficient that is not finite, or d' <= 0 with u given. PWW_ENOTSUP: `src` or (with u given) `out` of an unknown type; n of 2^36 or more.
 */
int pww_step_fwd(float *x, float *h, const void *m0, const void *m1, float g, const float *z, void *u, const float *row, int64_t n,
                 int32_t copies, int32_t src, int32_t out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_STEP_H */
