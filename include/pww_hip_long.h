/*
 * libpww_hip_long.so -- the cross-attention launches of PROMPTS LONGER THAN 77 TOKENS (chunked prompt encoding: 2 or 3 chunks of 77,
 * M = 154 / 231 keys; any 128 < M <= 256 is taken). A second shared object beside libpww_hip.so (include/pww_hip.h), built from the same
 * csrc/ headers for gfx950 (MI355X), loaded by the Python package on the first long-prompt call. It shares the descriptor structs, the
 * PWW_* return codes, dtype and statistic selectors of pww_hip.h and nothing else: every symbol here carries the prefix pww_long_, so
 * that a program may link both libraries.
 *
 * The arithmetic is paint_with_words/paint_with_words.py:87-116 of the reference, as in pww_hip.h:
 *     O = softmax((Q K^T + c[b] * bias) * scale) V,     c[b] = coeff_scalar * stat(Q K^T of image b) * gate[b]
 * split like the product path for <= 128 keys: a small launch forms partials of the per-image statistic over the finished Q
 * (pww_long_qk_parts), the attention launch folds them at entry (pww_long_cross_attn_fwd_parts); the kernel boundary is the only
 * synchronisation -- no atomics, nothing waits for another workgroup, results are bitwise repeatable.
 *
 * All functions return PWW_OK or a negative PWW_E* code; pww_long_last_error() describes the last failure of the calling thread.
 * Arguments are validated in front of the first HIP runtime call.
 */
#ifndef PWW_HIP_LONG_H
#define PWW_HIP_LONG_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_LONG_VERSION 100   /* major * 100 + minor of THIS library's ABI */
#define PWW_LONG_MIN_KEYS 129
#define PWW_LONG_MAX_KEYS 256

int pww_long_version(void);
const char *pww_long_last_error(void);

/*
 * Partials of the score statistic over a finished Q for 128 < M <= 256: the format of pww_qk_parts -- double [B][nparts][4] =
 * { max, min, sum, sum of squares }, only the fields `stat_kind` is made of, the others hold the neutral element -- with
 * nparts = pww_long_qk_parts_count(desc) <= 256 per image whenever H * ceil(N / 32) <= 256 * 4 * 64.
 * One wave per (image, head, 32-row block, 32-key block) and a partial per wave while that gives at most 256 partials per image; beyond,
 * a wave walks the (at most 8) key blocks of its row blocks, the next block's K fragments in flight under the current block's MFMAs, and
 * the four waves of a workgroup share one partial.
 *   q, k          as described by the attention descriptor: dtype, B / H / N / M / D and the q / k strides are read
 *   gate          fp32 [B] or NULL: images with gate[b] == 0 get no partials (their rows of `partials` are left untouched)
 *   gated_images  hint that gate[b] != 0 exactly for b < gated_images: the grid then covers those images only. 0 = every image may have
 *                 a non-zero gate (negative regions bias the unconditional rows too): the grid covers all B
 *   partials      16-byte aligned, partials_bytes >= B * nparts * 32
 * Sums accumulate in fp32 over a lane's 16 scores and in fp64 from there: within 1e-6, relative to the largest score, of pww_qk_reduce.
 */
int pww_long_qk_parts(const void *q, const void *k, const float *gate, const pww_attn_desc_t *desc, int32_t stat_kind, int32_t gated_images,
                      double *partials, size_t partials_bytes, void *stream);
int32_t pww_long_qk_parts_count(const pww_attn_desc_t *desc);

/*
 * The contract of pww_cross_attn_fwd_parts for 128 < M <= 256:
 *   c[b] = coeff_scalar * stat(fold(partials[b][0 .. nparts-1])) * gate[b]
 * `stats_out` (optional, double [B][4]) receives the folded fields. Of `opts` (NULL: none) coeff_scalar_dev (a device word that replaces
 * coeff_scalar when the kernel runs: one captured hipGraph for all denoise steps), bias_cols (columns >= bias_cols of the map are zero)
 * and gated_images are read; the compact form of the map is not taken (PWW_ENOTSUP). gate[b] may be any finite value (a factor of the
 * image's coefficient; exactly 0 = the image takes no bias and reads no partials), and gated_images == 0 means every image is biased.
 * bias: a dense fp32 map with unit key stride (bias_stride[3] == 1), required. D a multiple of 8 up to PWW_MAX_HEAD_DIM, f16 / bf16, any N.
 * One 128-row query block per workgroup; K / V in 128-key stages through LDS (both resident for D <= 96, walked in turn above), the wave's
 * bias rows staged per 64-key tile, the online softmax steps between tiles.
 */
int pww_long_cross_attn_fwd_parts(const void *q, const void *k, const void *v, void *o, const float *bias, int32_t stat_kind,
                                  float coeff_scalar, const float *gate, const pww_attn_desc_t *desc, const double *partials,
                                  int32_t nparts, double *stats_out, const pww_cross_opts_t *opts, void *stream);

/*
 * pww_cross_attn_probs for 128 < M <= 256 (same arguments, same one-owner-per-element accumulation): the head-averaged softmax
 * probabilities of one cross-attention call, for the attention-map recorder.
 */
int pww_long_cross_attn_probs(const void *q, const void *k, const float *bias, const double *stats, int32_t stat_kind, double stat_count,
                              float coeff_scalar, const float *gate, const pww_attn_desc_t *desc, const pww_cross_opts_t *opts, float *out,
                              const pww_probs_desc_t *pdesc, void *stream);

/*
 * Kernel-only timing of THIS library's launches, as pww_profile_arm / pww_profile_elapsed_us: the next launch of the arming thread is
 * stamped with the dispatch's own start / end; one slot at a time.
 */
int pww_long_profile_arm(void);
int pww_long_profile_elapsed_us(float *us);

#ifdef __cplusplus
}
#endif
#endif
