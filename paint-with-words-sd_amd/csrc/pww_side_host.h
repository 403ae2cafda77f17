// Host plumbing of a side library (libpww_hip_long.so, _scope, _linear, _regions, _lora): the few host helpers pww_common.h declares, defined once
// per library. A side library's one translation unit includes this exactly once, after
//
//   #define PWW_SIDE_LIB "libpww_hip_<x>"
//
// Nothing is shared with libpww_hip.so at link time: the unit is compiled with -fvisibility=hidden, so these definitions stay inside the
// library and only its pww_<x>_* entry points are visible. (pww_api.hip keeps the product library's own plumbing: its arch_ok reports the
// device's name, and its profile pool is a different thing.) Host code only -- nothing here reaches a kernel.
#pragma once
#ifndef PWW_SIDE_LIB
#error "define PWW_SIDE_LIB (the library's name, e.g. \"libpww_hip_long\") before including pww_side_host.h"
#endif
#include <string.h>
#include "pww_common.h"

namespace pww {

// the library's error slot, one per thread, and the accessor its pww_<x>_last_error entry point returns
static thread_local char g_side_err[512] = "";
static const char *last_error() { return g_side_err; }

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_side_err, sizeof(g_side_err), fmt, ap);
    va_end(ap);
}

int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return PWW_OK;
    set_error("%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    return PWW_EHIP;
}

bool arch_ok() {
    static thread_local int cached = -1;
    if (cached < 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (check_hip(hipGetDevice(&dev), "hipGetDevice") || check_hip(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties")) return false;
        cached = strncmp(prop.gcnArchName, "gfx950", 6) == 0 && (prop.gcnArchName[6] == 0 || prop.gcnArchName[6] == ':') ? 1 : 0;
    }
    if (!cached) set_error(PWW_SIDE_LIB " is built for gfx950 (MI355X) only");
    return cached == 1;
}

#ifndef PWW_SIDE_OWN_PROFILE
// (no timing slot: the library's launches are timed with event pairs or a profiler. A unit that has one defines PWW_SIDE_OWN_PROFILE
// and its own profile_take.)
bool profile_take(hipEvent_t *, hipEvent_t *, hipStream_t) { return false; }
#endif

static bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

}  // namespace pww
