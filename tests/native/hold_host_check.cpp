// Stand-alone host check of libpww_hip_hold's argument validation and of its two host tables (tests/test_hold_host.py compiles this file
// TOGETHER with csrc/pww_hold.hip, host side under -fsanitize=address,undefined, and runs it). Every launching call below must return in
// front of the first HIP runtime call: the pointers are never dereferenced by the device and no device is needed. Exit code 0 and
// "hold_host_check OK" = every case answered as expected and the sanitizers saw nothing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/pww_hip_hold.h"

static int failures = 0;

static void expect(int got, int want, const char *word, const char *what) {
    const char *err = pww_hold_last_error();
    if (got != want || (word && !strstr(err, word))) {
        printf("FAIL %s: rc %d (want %d), error \"%s\" (want \"%s\")\n", what, got, want, err, word ? word : "");
        ++failures;
    }
}

int main() {
    alignas(16) static char buf[64];
    void *p = buf;
    float *f = reinterpret_cast<float *>(buf), *f2 = f + 4;
    const uint8_t colors[PWW_HOLD_MAX_COLORS * 3] = {0};
    float deltas[PWW_HOLD_MAX_COLORS] = {0.f, 0.25f, -0.5f, 0.f, 0.f, 0.f, 0.f, 1.f};
    const float inf = INFINITY, nan = NAN;

    if (pww_hold_version() != PWW_HOLD_VERSION) { printf("FAIL version\n"); ++failures; }

    // ---- the strength map
    expect(pww_hold_strength_map(nullptr, colors, deltas, 0.5f, f, 64, 64, 1, nullptr), PWW_EINVAL, "required", "map rgb null");
    expect(pww_hold_strength_map(p, nullptr, deltas, 0.5f, f, 64, 64, 1, nullptr), PWW_EINVAL, "required", "map colors null");
    expect(pww_hold_strength_map(p, colors, nullptr, 0.5f, f, 64, 64, 1, nullptr), PWW_EINVAL, "required", "map deltas null");
    expect(pww_hold_strength_map(p, colors, deltas, 0.5f, nullptr, 64, 64, 1, nullptr), PWW_EINVAL, "required", "map out null");
    expect(pww_hold_strength_map(p, colors, deltas, 0.5f, f, 64, 64, 0, nullptr), PWW_EINVAL, "0 colours", "map K = 0");
    expect(pww_hold_strength_map(p, colors, deltas, 0.5f, f, 64, 64, 9, nullptr), PWW_EINVAL, "9 colours", "map K = 9");
    expect(pww_hold_strength_map(p, colors, deltas, 0.5f, f, 7, 64, 1, nullptr), PWW_EINVAL, "smaller than one latent pixel", "map H = 7");
    expect(pww_hold_strength_map(p, colors, deltas, 0.5f, f, 64, 0, 1, nullptr), PWW_EINVAL, "smaller than one latent pixel", "map W = 0");
    expect(pww_hold_strength_map(p, colors, deltas, nan, f, 64, 64, 1, nullptr), PWW_EINVAL, "not finite", "map s0 NaN");
    deltas[7] = inf;
    expect(pww_hold_strength_map(p, colors, deltas, 0.5f, f, 64, 64, 8, nullptr), PWW_EINVAL, "colour 7", "map delta inf");
    deltas[7] = 1.f;
    expect(pww_hold_strength_map(p, colors, deltas, 0.5f, f, 1 << 20, 1 << 20, 1, nullptr), PWW_ENOTSUP, "2^31", "map too large");

    // ---- the feather
    expect(pww_hold_feather(nullptr, f2, f, 8, 8, 1.f, nullptr), PWW_EINVAL, "required", "feather in null");
    expect(pww_hold_feather(f, nullptr, f, 8, 8, 1.f, nullptr), PWW_EINVAL, "required", "feather tmp null");
    expect(pww_hold_feather(f, f2, nullptr, 8, 8, 1.f, nullptr), PWW_EINVAL, "required", "feather out null");
    expect(pww_hold_feather(f, f, f2, 8, 8, 1.f, nullptr), PWW_EINVAL, "of its own", "feather tmp = in");
    expect(pww_hold_feather(f, f2, f2, 8, 8, 1.f, nullptr), PWW_EINVAL, "of its own", "feather tmp = out");
    expect(pww_hold_feather(f, f2, f, 0, 8, 1.f, nullptr), PWW_EINVAL, "bad size", "feather h = 0");
    expect(pww_hold_feather(f, f2, f, 8, -1, 1.f, nullptr), PWW_EINVAL, "bad size", "feather w < 0");
    expect(pww_hold_feather(f, f2, f, 8, 8, -0.5f, nullptr), PWW_EINVAL, "sigma", "feather sigma < 0");
    expect(pww_hold_feather(f, f2, f, 8, 8, 8.5f, nullptr), PWW_EINVAL, "sigma", "feather sigma > 8");
    expect(pww_hold_feather(f, f2, f, 8, 8, nan, nullptr), PWW_EINVAL, "sigma", "feather sigma NaN");
    expect(pww_hold_feather(f, f2, f, 8, 8, inf, nullptr), PWW_EINVAL, "sigma", "feather sigma inf");
    expect(pww_hold_feather(f, f2, f, 1 << 16, 1 << 16, 1.f, nullptr), PWW_ENOTSUP, "2^31", "feather too large");

    // ---- the hold
    for (int k = 0; k < 4; ++k) {
        float *a[4] = {f, f, f, f};
        a[k] = nullptr;
        expect(pww_hold_apply(a[0], a[1], a[2], a[3], 0.5f, 1.f, 1.f, 1, 4, 64, nullptr), PWW_EINVAL, "required", "apply null pointer");
    }
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, 1.f, 0, 4, 64, nullptr), PWW_EINVAL, "bad size", "apply n = 0");
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, 1.f, 1, 0, 64, nullptr), PWW_EINVAL, "bad size", "apply C = 0");
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, 1.f, 1, 4, 0, nullptr), PWW_EINVAL, "bad size", "apply hw = 0");
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, 1.f, 1, 4, -64, nullptr), PWW_EINVAL, "bad size", "apply hw < 0");
    expect(pww_hold_apply(f, f, f, f, nan, 1.f, 1.f, 1, 4, 64, nullptr), PWW_EINVAL, "finite", "apply theta NaN");
    expect(pww_hold_apply(f, f, f, f, 0.5f, inf, 1.f, 1, 4, 64, nullptr), PWW_EINVAL, "finite", "apply a inf");
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, -inf, 1, 4, 64, nullptr), PWW_EINVAL, "finite", "apply b -inf");
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, 1.f, 1, 1024, (int64_t)1 << 30, nullptr), PWW_ENOTSUP, "2^40", "apply 2^40 elements");
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, 1.f, 2, 1, (int64_t)1 << 30, nullptr), PWW_ENOTSUP, "2^31", "apply 2^31 pixels");
    expect(pww_hold_apply(f, f, f, f, 0.5f, 1.f, 1.f, 1, 4, (int64_t)1 << 40, nullptr), PWW_ENOTSUP, "2^40", "apply hw past int32");

    // ---- the tap table: radius = ceil(3 sigma), taps[0] = 1, descending, the formula in double
    float taps[PWW_HOLD_MAX_RADIUS + 2];
    const float sigmas[] = {0.f, 0.25f, 0.5f, 1.f, 2.f, 7.9f, 8.f};
    for (float s : sigmas) {
        for (float &t : taps) t = -1.f;
        const int radius = pww_hold_taps(s, taps, PWW_HOLD_MAX_RADIUS + 1);
        const int want = s > 0.f ? (int)ceil(3.0 * (double)s) : 0;
        if (radius != want || radius > PWW_HOLD_MAX_RADIUS || taps[0] != 1.f || taps[radius + 1] != -1.f) {
            printf("FAIL taps sigma %g: radius %d (want %d), taps[0] %g, behind the last %g\n", (double)s, radius, want, (double)taps[0], (double)taps[radius + 1]);
            ++failures;
        }
        for (int x = 1; x <= radius; ++x) {
            const float t = (float)exp(-0.5 * ((double)x / (double)s) * ((double)x / (double)s));
            if (taps[x] != t || !(taps[x] < taps[x - 1]) || !(taps[x] > 0.f)) { printf("FAIL taps sigma %g at %d: %g\n", (double)s, x, (double)taps[x]); ++failures; }
        }
    }
    expect(pww_hold_taps(8.f, taps, 24), PWW_EINVAL, "room for 24", "taps short buffer");
    expect(pww_hold_taps(2.f, nullptr, 25), PWW_EINVAL, "required", "taps null");
    expect(pww_hold_taps(nan, taps, 25), PWW_EINVAL, "sigma", "taps NaN");
    expect(pww_hold_taps(8.01f, taps, 25), PWW_EINVAL, "sigma", "taps sigma > 8");
    if (pww_hold_taps(2.f, taps, 7) != 6) { printf("FAIL taps: a buffer of exactly radius + 1 floats\n"); ++failures; }

    // ---- the threshold table: theta[0] = 1, theta[T] = 0, strictly descending, k / T in fp32
    static float theta[1001 + 1];
    const int steps[] = {1, 2, 3, 8, 30, 50, 100, 1000};
    for (int T : steps) {
        for (float &t : theta) t = -1.f;
        expect(pww_hold_thresholds(T, theta), PWW_OK, nullptr, "thresholds");
        if (theta[0] != 1.f || theta[T] != 0.f || theta[T + 1] != -1.f) { printf("FAIL thresholds T = %d: ends %g %g %g\n", T, (double)theta[0], (double)theta[T], (double)theta[T + 1]); ++failures; }
        for (int g = 1; g <= T; ++g)
            if (!(theta[g] < theta[g - 1]) || theta[g] != (float)((double)(T - g) / (double)T)) { printf("FAIL thresholds T = %d at %d\n", T, g); ++failures; }
    }
    if (pww_hold_thresholds(8, theta) != PWW_OK || theta[4] != 0.5f || theta[6] != 0.25f || theta[7] != 0.125f) { printf("FAIL thresholds of 8 steps\n"); ++failures; }
    expect(pww_hold_thresholds(0, theta), PWW_EINVAL, "0 steps", "thresholds T = 0");
    expect(pww_hold_thresholds(PWW_HOLD_MAX_STEPS + 1, theta), PWW_EINVAL, "steps", "thresholds T too large");
    expect(pww_hold_thresholds(8, nullptr), PWW_EINVAL, "required", "thresholds null");

    if (failures) { printf("hold_host_check: %d failure(s)\n", failures); return 1; }
    printf("hold_host_check OK\n");
    return 0;
}
