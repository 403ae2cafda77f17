/*
 * libpww_hip_canvas.so -- canvases larger than the UNet's window (MultiDiffusion, Bar-Tal et al. 2023): the canvas latent is denoised as
 * overlapping windows of the model's native size, and the per-pixel weighted mean of the windows' noise predictions takes one scheduler
 * step on the canvas. Two launches around the UNet evaluation of a step: the gather of the windows from the canvas, and the combine of the
 * windows' rows into one canvas-sized noise prediction. A shared object of its own beside libpww_hip.so (include/pww_hip.h) and the other
 * side libraries, built from csrc/pww_canvas.hip for gfx950 (MI355X) and loaded by the Python package on the first canvas request. It
 * shares the PWW_* return codes and dtype selectors of pww_hip.h and the bound PWW_REGIONS_MAX of pww_hip_regions.h, and nothing else;
 * every symbol carries the prefix pww_canvas_.
 *
 * Device pointers are owned by the caller; every function only enqueues on `stream` and is legal under stream capture; no atomics, nothing
 * waits for another workgroup, plain vector stores only, results are bitwise repeatable. The unit is compiled without FMA contraction and
 * every operation below is a single IEEE fp32 operation in the order written, so a CPU restatement in fp32 matches bit for bit. Arguments are
 * validated in front of the first HIP runtime call. pww_canvas_last_error() describes the last failure of the calling thread.
 *
 * The window grid. Along an axis of latent length L with window length win, the origins are an ascending HOST int32 array (they travel in
 * the kernel arguments): the first is 0, the last is L - win, and two consecutive origins are at most win apart, so every canvas pixel is
 * covered. (ops.canvas_windows: 0, s, 2 s, ... below L - win, then L - win -- the last window is clamped to the end, so its origin may be
 * odd and its overlap larger.) The windows are the product grid ys x xs; window iy * nx + ix has its origin at (ys[iy], xs[ix]). Both entry
 * points check all of this and return PWW_EINVAL otherwise.
 */
#ifndef PWW_HIP_CANVAS_H
#define PWW_HIP_CANVAS_H

#include "pww_hip.h"
#include "pww_hip_regions.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_CANVAS_VERSION 100      /* major * 100 + minor of THIS library's ABI */
#define PWW_CANVAS_MAX_WINDOWS 64   /* windows per canvas (ny * nx) */
#define PWW_CANVAS_MAX_RAMP 64      /* ramp length in latent pixels */
#define PWW_CANVAS_MIN_WINDOW 8     /* window height and width in latent pixels: 8 ... */
#define PWW_CANVAS_MAX_WINDOW 128   /* ... 128 */
#define PWW_CANVAS_MAX_CHANNELS 1024

int pww_canvas_version(void);
const char *pww_canvas_last_error(void);

/*
 * The windows of one step, as the rows of the UNet's input.
 *   canvas  device, fp32 [C][Hc][Wc]
 *   out     device, T [copies][ny nx][C][h][w]
 *   ys, xs  HOST, int32 [ny], [nx]
 * out[copy][iy nx + ix][c][ly][lx] = round_T(canvas[c][ys[iy] + ly][xs[ix] + lx] / denom): one fp32 division, then one rounding to T (to
 * nearest even); every copy holds the same values (the row classes of a folded call: prompt, region prompts, unconditional). One launch.
 * 16-byte stores when w is a multiple of 8 and out is 16-byte aligned, else one element per lane; the canvas is read with 4-byte loads
 * either way (an odd origin makes its rows unaligned). PWW_EINVAL: null pointers, a window grid that fails the checks above, h or w outside
 * 8 .. 128 or larger than the canvas, C outside 1 .. 1024, copies outside 1 .. PWW_REGIONS_MAX + 2, a denom that is not finite and
 * positive; PWW_ENOTSUP: a dtype other than PWW_DTYPE_F16 / PWW_DTYPE_BF16.
 */
int pww_canvas_gather(const float *canvas, void *out, const int32_t *ys, int32_t ny, const int32_t *xs, int32_t nx, int32_t C, int32_t Hc,
                      int32_t Wc, int32_t h, int32_t w, float denom, int32_t copies, int32_t dtype, void *stream);

/*
 * The noise prediction of the canvas from the windows' rows. With n_w = ny nx:
 *   eps     device, T [(K + 2)][n_w][C][h][w]   the UNet's output: rows [base x n_w, region 1 x n_w, ..., region K x n_w, unconditional x n_w]
 *   masks   device, fp32 [n_w][K][h w]          pww_regions_masks of every window's crop of the colour map
 *   weights device, fp32 [n_w][K]               a_k of pww_regions_combine, per window
 *   scales  device, fp32 [n_w][K]               s_k, per window
 *   out     device, fp32 [C][Hc][Wc]
 * masks, weights and scales are ignored (and may be null) when K = 0. Gather form: every canvas pixel (y, x) walks the windows that cover
 * it in ascending window index, with (ly, lx) = (y - ys[iy], x - xs[ix]):
 *   acc = 0;  ps = 0;
 *   per covering window:   acc = acc + p * v;   ps = ps + p;
 *   out = acc / ps
 * where, of that window's rows at (ly, lx),
 *   K = 0:   v = e_u + g * (e_0 - e_u)
 *   K >= 1:  w_k = a_k * M_k;   w_0 = 1 - (((w_1 + w_2) + ...) + w_K);   c_0 = w_0 * g;   c_k = w_k * s_k;
 *            v = (((e_u + c_0 * (e_0 - e_u)) + c_1 * (e_1 - e_u)) + ...) + c_K * (e_K - e_u)          (pww_regions_combine's expression)
 * and p = (float)(r_h(ly) * r_w(lx)) with r_L(l) = 1 when ramp = 0, else r_L(l) = min(min(l, L - 1 - l) + 1, ramp): an integer of at most
 * 4096, exact in fp32 and never zero. (ramp = 1 is ramp = 0.) p and the c_k are formed once per pixel and window and reused over the
 * channels, which are walked four at a time (a UNet's noise prediction has four). One launch. 16-byte loads and stores when w, Wc and every
 * origin of xs are multiples of 8 and every pointer is 16-byte aligned, else one pixel per lane. PWW_EINVAL: null pointers, a window grid
 * that fails the checks above, h or w outside 8 .. 128 or larger than the canvas, C outside 1 .. 1024, K outside 0 .. PWW_REGIONS_MAX,
 * ramp outside 0 .. PWW_CANVAS_MAX_RAMP; PWW_ENOTSUP: a dtype other than PWW_DTYPE_F16 / PWW_DTYPE_BF16.
 */
int pww_canvas_combine(const void *eps, const float *masks, const float *weights, const float *scales, float g, float *out,
                       const int32_t *ys, int32_t ny, const int32_t *xs, int32_t nx, int32_t K, int32_t C, int32_t Hc, int32_t Wc, int32_t h,
                       int32_t w, int32_t ramp, int32_t dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_CANVAS_H */
