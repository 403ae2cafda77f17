// The 160-wide tile of the plain 3 x 3 convolution (libpww_hip_convwide.so, include/pww_hip_convwide.h): pww_conv.hip compiled for that
// width alone. libpww_hip.so sits under its size limit by less than the tile's two code objects (13.4 KB each and their metadata), so
// they live here; kernel, plan (plan_conv) and table (CONV_TUNED) are the one source both libraries compile, and a descriptor is launched
// by exactly one of them: this one where the plan is the 160-wide tile, the product library everywhere else.
//
// The unit is self-contained: its host plumbing is pww_side_host.h, and only the pww_convwide_* entry points are visible (compiled with
// -fvisibility=hidden).
#define PWW_SIDE_LIB "libpww_hip_convwide"
#include "pww_side_host.h"
#include "../../include/pww_hip_convwide.h"

#define PWW_CONVWIDE_API extern "C" __attribute__((visibility("default")))

#define PWW_CONV_WIDE_UNIT 1
#include "pww_conv.hip"

PWW_CONVWIDE_API int pww_convwide_version(void) { return PWW_CONVWIDE_VERSION; }
PWW_CONVWIDE_API const char *pww_convwide_last_error(void) { return pww::last_error(); }
PWW_CONVWIDE_API int pww_convwide_takes(const pww_conv_desc_t *desc) { return pww::conv3x3_plans_wide(desc); }
PWW_CONVWIDE_API size_t pww_convwide_workspace_bytes(const pww_conv_desc_t *desc) { return pww::conv3x3_workspace_bytes(desc); }
PWW_CONVWIDE_API int pww_convwide_fwd(const void *x, const void *w, const void *bias, const void *residual, void *y, const pww_conv_desc_t *desc,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    return pww::conv3x3_fwd(x, w, bias, residual, y, desc, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
