/*
 * libpww_hip_vaeenc.so -- the three pieces of the AutoencoderKL encoder that no other kernel of this project covers: the head (image ->
 * conv_in, 3 input channels), the downsamplers (3 x 3, stride 2, zero padding on the right and bottom only) and the tail (conv_norm_out ->
 * SiLU -> conv_out to 8 channels -> quant_conv -> mean / logvar -> the scaled latent). A side library beside libpww_hip.so
 * (include/pww_hip.h), built from csrc/pww_vaeenc.hip for gfx950 (MI355X) and loaded by the Python package on the first call that needs it
 * (pww_hip/vae_encode.py). It shares the PWW_* return codes and dtype selectors of pww_hip.h and nothing else; every symbol carries the
 * prefix pww_vaeenc_.
 *
 * Device pointers are owned by the caller; the functions only enqueue on `stream` and are legal under stream capture; no atomics, nothing
 * waits for another workgroup, vector stores only, results are bitwise repeatable. Arguments are validated in front of the first HIP runtime
 * call. pww_vaeenc_last_error() describes the last failure of the calling thread.
 */
#ifndef PWW_HIP_VAEENC_H
#define PWW_HIP_VAEENC_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_VAEENC_VERSION 100          /* major * 100 + minor of THIS library's ABI; the descriptors also carry their own size */
#define PWW_VAEENC_IN_SAMPLE 0          /* [B][3][H][W] in the storage type: what vae.encode is given */
#define PWW_VAEENC_IN_UINT8 1           /* [B][H][W][3] uint8 pixels + the 256-entry table of their normalised values */
#define PWW_VAEENC_HEAD_CHANNELS 128
#define PWW_VAEENC_TAIL_CHANNELS 512
#define PWW_VAEENC_TAIL_GROUPS 32
#define PWW_VAEENC_TAIL_MAX_CHUNKS 64

int pww_vaeenc_version(void);
const char *pww_vaeenc_last_error(void);

/*
 * The head: y = conv3x3(v, w) + bias, padding 1, 3 -> 128 channels, written channels_last ([B][H][W][128], the storage type T).
 *   PWW_VAEENC_IN_SAMPLE   v = image[b][c][h][w]                     (T)
 *   PWW_VAEENC_IN_UINT8    v = table[image[b][h][w][c]]              (`table`: 256 values of T, made by the caller with the very expression
 *                                                                    that normalises a pixel, so the two forms see the same bits)
 * The zero padding is of v: a tap outside the image contributes 0 (not pixel 0, which normalises to -1). The 27 products of a T value and a
 * T weight are exact in fp32; they are summed in fp32 in one fixed order (one mfma_f32_16x16x32 with the contraction padded from 27 to 32
 * by zeros), and the result is rounded ONCE: y = T(acc + bias). (A stock convolution followed by a bias add in T rounds twice.)
 *   w  [128][3][3][3] contiguous (T): conv_in.weight           bias  [128] (T)
 * Any H, W >= 1.
 * PWW_EINVAL:  a null pointer (`table` only with the uint8 form), a descriptor shorter than this struct, B / H / W < 1.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, `in` other than the two forms, image, w or y not 16-byte aligned (the uint8 image: any), an
 *              output of 2^31 elements or more, a device other than gfx950.
 */
typedef struct pww_vaeenc_head_desc {
    uint32_t size;          /* sizeof(pww_vaeenc_head_desc_t) */
    int32_t dtype;          /* PWW_DTYPE_* */
    int32_t B, H, W;
    int32_t in;             /* PWW_VAEENC_IN_* */
} pww_vaeenc_head_desc_t;
int pww_vaeenc_head_fwd(const void *image, const void *table, const void *w, const void *bias, void *y, const pww_vaeenc_head_desc_t *desc,
                        void *stream);

/*
 * A downsampler: 3 x 3 convolution with stride 2 over F.pad(x, (0, 1, 0, 1)) -- zero padding on the right and bottom only, so output
 * (oy, ox) reads the taps at 2 o + {0, 1, 2} -- channels_last in and out ([B][H][W][Cin] -> [B][Ho][Wo][Cout]), Ho = (H - 2) / 2 + 1,
 * Wo likewise. H, W >= 2; at an odd size no padding is read. It is the implicit GEMM of pww_conv3x3_fwd (csrc/pww_conv.hip compiled into
 * this library with the pad origin at 0): the same tiles (tile_n 64 or 128, 0: the library's choice), the same split of K with a fold
 * launch (splitk, 0: the library's choice; needs the workspace), the same epilogue T(T(acc) + bias).
 *   w  [Cout][3][3][Cin] (the storage of a channels_last nn.Conv2d weight)            bias  [Cout] or null
 * PWW_EINVAL:  a null pointer, a descriptor shorter than this struct, a workspace that is too small.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, B < 1, H or W < 2, Cin or Cout no multiple of 64, a tile_n other than 0 / 64 / 128 or one that
 *              does not divide Cout, a split above the K-slabs, a tensor of 2^31 elements or more, a device other than gfx950.
 */
typedef struct pww_vaeenc_down_desc {
    uint32_t size;          /* sizeof(pww_vaeenc_down_desc_t) */
    int32_t dtype;          /* PWW_DTYPE_* */
    int32_t B, H, W, Cin, Cout;
    int32_t tile_n, splitk; /* 0: the library's choice */
} pww_vaeenc_down_desc_t;
size_t pww_vaeenc_down_workspace_bytes(const pww_vaeenc_down_desc_t *desc);
int pww_vaeenc_down_fwd(const void *x, const void *w, const void *bias, void *y, const pww_vaeenc_down_desc_t *desc, void *workspace,
                        size_t workspace_bytes, void *stream);

/*
 * The tail, for a channels_last x [B][512][h][w] (memory [B][h][w][512]):
 *   m = quant(conv3x3(SiLU(GroupNorm_32(x)), w) + bias)          quant: the 1 x 1 convolution qw [8][8], qb [8]
 *   mean = m[0..3]     logvar = min(max(m[4..7], -30), 20)
 *   moments[b][0..3][h][w] = mean, moments[b][4..7][h][w] = logvar                           (fp32; optional: null skips it)
 *   z[b][i][h][w] = scale * (mean_i + exp(logvar_i / 2) * noise[b][i][h][w])                  (fp32; noise null: scale * mean_i)
 * The convolution's zero padding applies to the activation: a tap outside the image contributes 0. From the normalised value to the outputs
 * everything is fp32: nothing in between is rounded to the storage type.
 * Two launches. pww_vaeenc_tail_stats forms, per image, chunk of pixels and group, the fp32 sum and sum of squares of x in a fixed order
 * (and, when `w` is given, the fp32 copy of the weight the second launch reads) in `ws`; the same input gives the same bytes. The second
 * launch adds the chunks up in their order, normalises, and convolves. pww_vaeenc_tail_fwd enqueues both; `ws` needs
 * pww_vaeenc_tail_workspace_bytes.
 *   gamma, beta  [512] (storage type)      w  [8][512][3][3] contiguous      bias  [8]      qw  [8][8]      qb  [8]      noise  [B][4][h][w]
 * Any h, w >= 1.
 * PWW_EINVAL:  a null pointer (but noise, moments), a descriptor shorter than this struct, B / H / W < 1, a workspace that is too small.
 * PWW_ENOTSUP: a dtype other than F16 / BF16, C != 512, eps <= 0, x not 16-byte aligned, a tensor of 2^31 elements or more, more than
 *              65535 images or row tiles, a device other than gfx950.
 */
typedef struct pww_vaeenc_tail_desc {
    uint32_t size;          /* sizeof(pww_vaeenc_tail_desc_t) */
    int32_t dtype;          /* PWW_DTYPE_* */
    int32_t B, H, W, C;     /* C: 512 */
    float eps;
    float scale;
} pww_vaeenc_tail_desc_t;
size_t pww_vaeenc_tail_workspace_bytes(const pww_vaeenc_tail_desc_t *desc);
int pww_vaeenc_tail_chunks(const pww_vaeenc_tail_desc_t *desc);      /* chunks per image of the statistics launch (0: unsupported) */
int pww_vaeenc_tail_stats(const void *x, const void *w, const pww_vaeenc_tail_desc_t *desc, void *ws, size_t ws_bytes, void *stream);
int pww_vaeenc_tail_fwd(const void *x, const void *gamma, const void *beta, const void *w, const void *bias, const void *qw, const void *qb,
                        const void *noise, void *moments, void *z, const pww_vaeenc_tail_desc_t *desc, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PWW_HIP_VAEENC_H */
