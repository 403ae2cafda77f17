/*
 * libpww_hip_hold.so -- region strength: a denoising strength per colour of the colour map for img2img (Differential Diffusion, Levin and
 * Fried 2023). Every latent pixel carries a strength S in [0, 1]; a pixel is released to the sampler at the step its strength allows and
 * is held at the noised init latent of the next step until then. A shared object of its own beside libpww_hip.so (include/pww_hip.h) and
 * the other side libraries, built from csrc/pww_hold.hip for gfx950 (MI355X) and loaded by the Python package on the first request that
 * names a region strength. It shares the PWW_* return codes of pww_hip.h and nothing else; every symbol carries the prefix pww_hold_.
 *
 * Device pointers are owned by the caller; every launching function only enqueues on `stream` and is legal under stream capture; no atomics,
 * nothing waits for another workgroup, plain vector stores only, results are bitwise repeatable. The unit is compiled without FMA
 * contraction and every operation below is a single IEEE fp32 operation in the order written, so a CPU restatement in fp32 matches bit for
 * bit. Arguments are validated in front of the first HIP runtime call. pww_hold_last_error() describes the last failure of the calling
 * thread.
 */
#ifndef PWW_HIP_HOLD_H
#define PWW_HIP_HOLD_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_HOLD_VERSION 100        /* major * 100 + minor of THIS library's ABI */
#define PWW_HOLD_MAX_COLORS 8       /* named colours per request */
#define PWW_HOLD_MAX_FEATHER 8.0f   /* sigma of the feather, in latent pixels */
#define PWW_HOLD_MAX_RADIUS 24      /* ceil(3 * PWW_HOLD_MAX_FEATHER): the feather has at most 2 * 24 + 1 taps */
#define PWW_HOLD_MAX_STEPS 100000   /* steps of a schedule pww_hold_thresholds tabulates */

int pww_hold_version(void);
const char *pww_hold_last_error(void);

/*
 * The strength map at latent resolution, h = H / 8, w = W / 8; rows and columns of the map past 8 h / 8 w are ignored.
 *   rgb     device, uint8 [H][W][3]
 *   colors  HOST, uint8 [K][3]     (they travel in the kernel arguments)
 *   deltas  HOST, fp32 [K]         d_k = s_k - s0, formed by the caller
 *   out     device, fp32 [h][w]
 * With c_k the number of pixels of the latent pixel's 8 x 8 block whose colour equals colors[k] exactly, and m_k = (float)c_k * (1 / 64)
 * (exact):
 *   S = ((s0 + m_1 * d_1) + m_2 * d_2) + ... + m_K * d_K;   out = min(max(S, 0), 1)
 * One launch, one latent pixel per lane. PWW_EINVAL: null pointers, K outside 1 .. PWW_HOLD_MAX_COLORS, H or W below 8, s0 or a delta that
 * is not finite; PWW_ENOTSUP: 2^31 latent pixels or more.
 */
int pww_hold_strength_map(const void *rgb, const uint8_t *colors, const float *deltas, float s0, float *out, int32_t H, int32_t W, int32_t K,
                          void *stream);

/*
 * A separable normalised Gaussian over one plane, along the rows (in -> tmp) and then along the columns (tmp -> out): two launches, both
 * planes in global memory, so there is no limit on the plane. The taps, their accumulation order and the normalisation at the edges are
 * those of pww_regions_masks (include/pww_hip_regions.h): taps exp(-0.5 (x / sigma)^2) for |x| <= ceil(3 sigma), formed in double on the
 * host and rounded to fp32 (pww_hold_taps), each pass accumulated in ascending x -- acc = acc + t * v, norm = norm + t, from 0 -- over the x
 * inside the plane and divided, acc / norm. A plane with values in [0, 1] stays in [0, 1]. sigma = 0 copies the plane.
 *   in, tmp, out   device, fp32 [h][w]; out may be in, tmp is neither
 * PWW_EINVAL: null pointers, tmp equal to in or out, h or w below 1, sigma negative, not finite or above PWW_HOLD_MAX_FEATHER;
 * PWW_ENOTSUP: 2^31 pixels or more.
 */
int pww_hold_feather(const float *in, float *tmp, float *out, int32_t h, int32_t w, float sigma, void *stream);

/*
 * The hold of one step, in place:   x = (S < theta) ? a * x0 + b * z : x      per image and pixel, over the C channels
 *   x       device, fp32 [n][C][hw]   the latent behind the scheduler's step
 *   x0, z   device, fp32 [n][C][hw]   the init latent and the request's noise
 *   S       device, fp32 [n][hw]      the strength map
 * A select, not a blend: a held pixel is overwritten whatever it held (a NaN too), a released pixel is not touched (not even rewritten).
 * The predicate is formed once per pixel and reused over the channels; the new value is two multiplications and one addition. One launch.
 * 16-byte loads and stores when hw is a multiple of 4 and every pointer is 16-byte aligned, else one pixel per lane. PWW_EINVAL: null
 * pointers, n, C or hw below 1, a theta, a or b that is not finite; PWW_ENOTSUP: x of 2^40 elements or more, S of 2^31 or more.
 */
int pww_hold_apply(float *x, const float *x0, const float *z, const float *S, float theta, float a, float b, int32_t n, int32_t C, int64_t hw,
                   void *stream);

/*
 * Host only (no HIP call): the two tables the launches above and their callers share.
 * pww_hold_taps: taps[x] for x = 0 .. radius of the feather of `sigma`, radius = ceil(3 sigma) (0, with taps[0] = 1, for sigma = 0);
 * returns the radius, or PWW_EINVAL (null pointer, sigma as refused by pww_hold_feather, cap < radius + 1 floats).
 * pww_hold_thresholds: theta[g] = (float)((double)(T - g) / (double)T) for g = 0 .. T (T + 1 floats): a pixel of strength S is released at
 * step g of T iff S >= theta[g]. PWW_EINVAL: null pointer, T outside 1 .. PWW_HOLD_MAX_STEPS.
 */
int pww_hold_taps(float sigma, float *taps, int32_t cap);
int pww_hold_thresholds(int32_t T, float *theta);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_HOLD_H */
