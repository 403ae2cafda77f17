/*
 * libpww_hip_regions.so -- region prompts: a full prompt per colour of the colour map, blended per latent pixel where classifier-free
 * guidance is combined ("latent couple"). A fifth shared object beside libpww_hip.so (include/pww_hip.h), libpww_hip_long.so,
 * libpww_hip_scope.so and libpww_hip_linear.so, built from csrc/pww_regions.hip for gfx950 (MI355X) and loaded by the Python package on the
 * first call that carries region prompts. It shares the PWW_* return codes and dtype selectors of pww_hip.h and nothing else; every symbol
 * carries the prefix pww_regions_.
 *
 * Device pointers are owned by the caller; every function only enqueues on `stream` and is legal under stream capture; no atomics, nothing
 * waits for another workgroup, plain vector stores only, results are bitwise repeatable. The unit is compiled without FMA contraction and
 * every operation below is a single IEEE fp32 operation in the order written, so a CPU restatement in fp32 matches bit for bit. Arguments are
 * validated in front of the first HIP runtime call. pww_regions_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_REGIONS_H
#define PWW_HIP_REGIONS_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_REGIONS_VERSION 100   /* major * 100 + minor of THIS library's ABI */
#define PWW_REGIONS_MAX 8         /* region prompts per image */
#define PWW_REGIONS_MAX_PLANE 9216    /* latent pixels of one mask plane (96 x 96: a 768 x 768 colour map) -- the plane lives in LDS */
#define PWW_REGIONS_MAX_FEATHER 8.0f  /* sigma of the feather, in latent pixels */

int pww_regions_version(void);
const char *pww_regions_last_error(void);

/*
 * Region masks at latent resolution: out[k][i][j] = the fraction of the 8 x 8 block of colour-map pixels under latent pixel (i, j) whose
 * colour equals colors[k] exactly (a multiple of 1 / 64), h = H / 8, w = W / 8; rows and columns of the map past 8 h / 8 w are ignored.
 *   rgb     device, uint8 [H][W][3]
 *   colors  HOST, uint8 [K][3] (they travel in the kernel arguments)
 *   out     device, fp32 [K][h][w]
 * feather > 0: a separable Gaussian over each plane, along the rows and then along the columns, taps exp(-0.5 (x / feather)^2) for
 * |x| <= ceil(3 feather) (formed in double on the host, rounded to fp32), each pass accumulated in ascending x and divided by the sum of the
 * taps that fall inside the plane, accumulated the same way: a constant plane stays constant and sum_k out[k] <= 1 survives up to rounding.
 * One workgroup per plane, one launch. PWW_EINVAL: null pointers, K outside 1 .. PWW_REGIONS_MAX, H or W below 8, feather negative, not finite
 * or above PWW_REGIONS_MAX_FEATHER; PWW_ENOTSUP: more than PWW_REGIONS_MAX_PLANE latent pixels.
 */
int pww_regions_masks(const void *rgb, int32_t H, int32_t W, const uint8_t *colors, int32_t K, float feather, float *out, void *stream);

/*
 * The blend of the noise predictions of one step. Rows of eps: [base x n, region 1 x n, ..., region K x n, unconditional x n].
 *   eps     device, T [(K + 2) n][C][hw]   the UNet's output, NCHW contiguous (hw = h * w)
 *   masks   device, fp32 [n][K][hw]        pww_regions_masks of every image
 *   weights device, fp32 [n][K]            a_k = weight_k (1 - base weight), formed by the caller
 *   scales  device, fp32 [n][K]            s_k, region k's guidance scale
 *   out     device, fp32 [n][C][hw]
 * Per image and pixel:   w_k = a_k * M_k;   w_0 = 1 - (((w_1 + w_2) + ...) + w_K);   c_0 = w_0 * g;   c_k = w_k * s_k;
 *   out = (((e_u + c_0 * (e_0 - e_u)) + c_1 * (e_1 - e_u)) + ...) + c_K * (e_K - e_u)
 * The coefficients are formed once per pixel and reused over the C channels. 16-byte loads and stores when hw is a multiple of 8 and every
 * pointer is 16-byte aligned, else one pixel per lane. PWW_EINVAL: null pointers, n outside 1 .. 65535, K outside 1 .. PWW_REGIONS_MAX,
 * C or hw below 1; PWW_ENOTSUP: a dtype other than PWW_DTYPE_F16 / PWW_DTYPE_BF16, eps of 2^40 elements or more.
 */
int pww_regions_combine(const void *eps, const float *masks, const float *weights, const float *scales, float g, float *out, int32_t n,
                        int32_t K, int32_t C, int64_t hw, int32_t dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_REGIONS_H */
