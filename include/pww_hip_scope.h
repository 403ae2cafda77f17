/*
 * libpww_hip_scope.so -- cross-attention whose bias coefficient is a PER-HEAD or PER-ROW statistic of the raw scores: the weight
 * functions  c * w * g(sigma) * qk.amax(dim=(1, 2), keepdim=True)  (each head scaled by its own statistic) and
 * c * w * g(sigma) * qk.std(dim=-1, keepdim=True)  (each query row scaled by the statistic of its own scores over the prompt tokens).
 * A third shared object beside libpww_hip.so (include/pww_hip.h) and libpww_hip_long.so, built from the same csrc/ headers for gfx950
 * (MI355X), loaded by the Python package on the first call that needs it. It shares the descriptor structs, the PWW_* return codes, the
 * dtype and statistic selectors of pww_hip.h and nothing else: every symbol here carries the prefix pww_scope_, so that a program may
 * link all three libraries.
 *
 * The arithmetic is paint_with_words/paint_with_words.py:87-116 of the reference:
 *     O = softmax((Q K^T + c * bias) * scale) V
 * with c per (image, head) or per (image, head, query row). Device pointers are owned by the caller; every function only enqueues on
 * `stream` and is legal under stream capture; no atomics, nothing waits for another workgroup, results are bitwise repeatable.
 *
 * All functions return PWW_OK or a negative PWW_E* code; pww_scope_last_error() describes the last failure of the calling thread.
 * Arguments are validated in front of the first HIP runtime call: a call that fails validation touches no pointer.
 *   PWW_ENOTSUP   M > 128, D not a multiple of 8 or above PWW_MAX_HEAD_DIM, a dtype other than f16 / bf16, a map without unit key
 *                 stride, slices of 2 GiB and more, a device that is not gfx950
 *   PWW_EINVAL    everything else: null / misaligned pointers, bad strides, a scope or statistic selector outside the lists below,
 *                 PWW_STAT_STD over a single score (M = 1 in row scope, N * M = 1 in head scope: NaN in torch), a partials buffer that
 *                 is too small, a partials count other than pww_scope_head_parts_count()
 */
#ifndef PWW_HIP_SCOPE_H
#define PWW_HIP_SCOPE_H

#include "pww_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PWW_SCOPE_VERSION 100   /* major * 100 + minor of THIS library's ABI */
#define PWW_SCOPE_MAX_KEYS 128

int pww_scope_version(void);
const char *pww_scope_last_error(void);

/*
 * Head scope only: partials of the raw scores per (image, head). The layout is PROMISED: double [B][H][P][4] = { max, min, sum, sum of
 * squares } with P = pww_scope_head_parts_count(desc) (<= 256 for every N; P = ceil(N / 128) up to N = 32768), only the fields
 * `stat_kind` is made of, the others hold the neutral element. One workgroup of four waves per partial: a wave forms the scores of its 32
 * query rows against every 32-key block by MFMA (fp32 sums over a lane's 16 scores, fp64 from there), the four waves meet in LDS in a fixed
 * order: within 1e-6, relative to the largest score, of the same reduction in fp64.
 *   q, k        as described by the attention descriptor: dtype, B / H / N / M / D and the q / k strides are read
 *   gate        fp32 [B] or NULL: gate[b] == 0 leaves that image's rows of `partials` untouched
 *   stat_kind   PWW_STAT_MAX / MIN / MEAN / STD / ABSMAX
 *   partials    16-byte aligned, partials_bytes >= B * H * P * 32
 * pww_scope_head_parts_count returns 0 for a problem the library does not take.
 */
int32_t pww_scope_head_parts_count(const pww_attn_desc_t *desc);
int pww_scope_head_parts(const void *q, const void *k, const float *gate, const pww_attn_desc_t *desc, int32_t stat_kind,
                         double *partials, size_t partials_bytes, void *stream);

/*
 * O = softmax((Q K^T + c * bias) * scale) V with
 *   scope HEAD: c[b][h]    = coeff * stat(fold(partials[b][h][0 .. P))) * gate[b]      (count of MEAN / STD: N * M)
 *   scope ROW : c[b][h][n] = coeff * stat(S[b][h][n][0 .. M))           * gate[b]      (no partials: pass NULL / 0; count: M)
 * coeff = *opts->coeff_scalar_dev if given (read when the kernel RUNS: one captured hipGraph serves every denoise step), else
 * coeff_scalar; the products are taken in fp32 in the order written. gate (fp32 [B] or NULL = 1) may be any finite value; exactly 0
 * means the image takes no bias and forms no statistic: its partials are never folded (the prologue's load batch may still request
 * those rows of the buffer, which pww_scope_head_parts left unwritten; the values are discarded) and its stats_out row stays untouched.
 * STD is unbiased, like torch.std: in head scope from the fp64 sum and sum of squares, in row scope centred in fp32 (mean first, then the
 * squared deviations: the row's scores are in registers).
 *   bias        fp32 map addressed through desc->bias_stride, unit key stride (bias_stride[3] == 1), required
 *   partials    HEAD: what pww_scope_head_parts wrote for the same q / k, nparts = pww_scope_head_parts_count(desc)
 *   stats_out   optional, HEAD only: double [B][H][4], the folded fields that were formed (rows of gated-out images untouched)
 *   opts        NULL or a pww_cross_opts_t: only coeff_scalar_dev is read
 * Supported: M <= 128, D a multiple of 8 up to PWW_MAX_HEAD_DIM, f16 / bf16, any N and B, k_stride[0] == 0 (a shared prompt).
 * One workgroup per (128 query rows, head, image): K and V of the head are staged once, a wave holds every score of its 32 rows in
 * registers (at most four 32-key blocks), so the row statistic is a reduction in registers and the softmax is one-shot (exact row
 * maximum, exp, row sum) -- no pre-pass for row scope, no online rescaling.
 */
#define PWW_SCOPE_HEAD 1
#define PWW_SCOPE_ROW 2
int pww_scope_cross_attn_fwd(const void *q, const void *k, const void *v, void *o, const float *bias, int32_t stat_kind, int32_t scope,
                             float coeff_scalar, const float *gate, const pww_attn_desc_t *desc, const double *partials, int32_t nparts,
                             double *stats_out, const pww_cross_opts_t *opts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
