// The second 3 x 3 convolution of a ResnetBlock2D that changes its channel count, with the block's 1 x 1 shortcut convolution as further
// K-slabs of the same implicit GEMM on gfx950 MFMA (pww_convtail_fwd):
//
//   y[m, n] = T( sum_k X[m, k] W[n, k]  +  sum_c X2[m, c] W2[n, c]  +  bias[n] + bias2[n] ),   m = (b, oy, ox),  k = (ky, kx, ci)
//
// The shortcut is a linear map summed into the same output, so the two sums are ONE GEMM with K' = 9 Cin + C2: the 1 x 1 convolution's own
// launch, the write of its output tensor and the epilogue's read of it as `residual` go away.
//
// The kernel, its fold, the measured plans (TAIL_TUNED) and the launch are pww_shortcut_gemm.h, shared with the two-source entry point of
// pww_concat.hip: here the kernel is instantiated with ONE part (C2) and this unit's cold struct. The measured times rest on the code
// objects, and how the source is shared decides whether they move: a `__device__` body behind `__global__` wrappers does move them, the
// `__global__` template itself does not -- all sixteen code objects of the two units are those of two written-out copies
// (profiles/shortcut_gemm.md). What is left here is what differs: the descriptor's checks with their texts, the pointer checks and the
// entry points.
//
// Built as a library of its own (libpww_hip_convtail.so, include/pww_hip_convtail.h): the unit is self-contained, its host plumbing is
// pww_side_host.h, and only the pww_convtail_* entry points are visible (compiled with -fvisibility=hidden).
#define PWW_SIDE_LIB "libpww_hip_convtail"
#include "pww_side_host.h"
#include "../../include/pww_hip_convtail.h"
#include "pww_shortcut_gemm.h"

#define PWW_CONVTAIL_API extern "C" __attribute__((visibility("default")))

namespace pww {

namespace {

// cold kernel arguments (behind the preloaded hot ones), in the field names of pww_shortcut_gemm.h: x1 / wsc are this entry point's x2 / w2
struct TailCold {
    const void *x1, *wsc, *bias, *bias2;
    int nsplit, nmain, ntail;
    int through;            // split launches: the partials are stored write-through (pww_common.h: store_partial_through)
};

bool plan_tail(const pww_convtail_desc_t *d, TailPlan *p) {
    if (!d || d->size < sizeof(pww_convtail_desc_t)) { set_error("convtail: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return false; }
    if ((d->dtype != PWW_DTYPE_F16 && d->dtype != PWW_DTYPE_BF16) || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 64 || d->Cin % 64 != 0 || d->C2 < 64
        || d->C2 % 64 != 0 || d->Cout < 64 || (d->Cout % 64 != 0 && d->Cout % 160 != 0) || d->Cin > 65536 || d->C2 > 65536 || d->Cout > 65536) {
        set_error("convtail: unsupported (dtype %d B %d %dx%d Cin %d C2 %d Cout %d): Cin and C2 multiples of 64, Cout of 64 or 160", d->dtype, d->B, d->H,
                  d->W, d->Cin, d->C2, d->Cout);
        return false;
    }
    const long M = (long)d->B * d->H * d->W;
    if (M * d->Cin >= (1L << 31) || M * d->C2 >= (1L << 31) || M * d->Cout >= (1L << 31) || 9L * d->Cin * d->Cout >= (1L << 31)
        || (long)d->C2 * d->Cout >= (1L << 31)) {
        set_error("convtail: tensor of 2^31 elements or more");
        return false;
    }
    return plan_tail("convtail", (int)M, 9 * d->Cin / 64, d->C2 / 64, d->Cout, d->tile_n, d->splitk, p);
}

}  // namespace

size_t convtail_workspace_bytes(const pww_convtail_desc_t *d) {
    TailPlan p;
    return plan_tail(d, &p) ? tail_workspace_bytes(p, d->Cout) : 0;
}

int convtail_fwd(const void *x, const void *w, const void *x2, const void *w2, const void *bias, const void *bias2, void *y, const pww_convtail_desc_t *d,
                 void *workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!d || d->size < sizeof(pww_convtail_desc_t)) { set_error("convtail: descriptor missing or older than this library (size %u)", d ? d->size : 0u); return PWW_EINVAL; }
    TailPlan p;
    if (!plan_tail(d, &p)) return PWW_ENOTSUP;
    if (!x || !w || !x2 || !w2 || !bias || !bias2 || !y) { set_error("convtail: x, w, x2, w2, bias, bias2 and y are required"); return PWW_EINVAL; }
    if (!aligned16(x) || !aligned16(w) || !aligned16(x2) || !aligned16(w2) || !aligned16(y) || (reinterpret_cast<uintptr_t>(bias) & 7)
        || (reinterpret_cast<uintptr_t>(bias2) & 7)) {
        set_error("convtail: x, w, x2, w2, y must be 16-byte aligned, the biases 8-byte aligned");
        return PWW_EINVAL;
    }
    const size_t need = tail_workspace_bytes(p, d->Cout);
    if (need && (!workspace || !aligned16(workspace) || workspace_bytes < need)) {
        set_error("convtail: split %d needs a 16-byte aligned workspace of %zu bytes (got %zu)", p.nsplit, need, workspace_bytes);
        return PWW_EINVAL;
    }
    if (!arch_ok()) return PWW_ENOTSUP;
    const TailCold cold{x2, w2, bias, bias2, 0, 0, 0, 0};       // (the plan's half is filled in by the launch)
    if (d->dtype == PWW_DTYPE_F16) return tail_launch<f16>("convtail", p, x, w, cold, y, workspace, d->Cout, d->Cin, d->H, d->W, stream, d->C2);
    return tail_launch<bf16>("convtail", p, x, w, cold, y, workspace, d->Cout, d->Cin, d->H, d->W, stream, d->C2);
}

}  // namespace pww

PWW_CONVTAIL_API int pww_convtail_version(void) { return PWW_CONVTAIL_VERSION; }
PWW_CONVTAIL_API const char *pww_convtail_last_error(void) { return pww::last_error(); }
PWW_CONVTAIL_API size_t pww_convtail_workspace_bytes(const pww_convtail_desc_t *desc) { return pww::convtail_workspace_bytes(desc); }
PWW_CONVTAIL_API int pww_convtail_fwd(const void *x, const void *w, const void *x2, const void *w2, const void *bias, const void *bias2, void *y,
                                      const pww_convtail_desc_t *desc, void *workspace, size_t workspace_bytes, void *stream) {
    return pww::convtail_fwd(x, w, x2, w2, bias, bias2, y, desc, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
