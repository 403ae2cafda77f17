// Stand-alone host check of libpww_hip_concat's argument validation (tests/test_concat_host.py compiles this file TOGETHER with
// csrc/pww_concat.hip, host side under -fsanitize=address,undefined, and runs it). Every call below must return in front of the first HIP
// runtime call: the pointers are never dereferenced and no device is needed. Exit code 0 and "concat_host_check OK" = every case answered
// as expected and the sanitizers saw nothing.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/pww_hip_concat.h"

static int failures = 0;

static void expect(int got, int want, const char *word, const char *what) {
    const char *err = pww_concat_last_error();
    if (got != want || (word && !strstr(err, word))) {
        printf("FAIL %s: rc %d (want %d), error \"%s\" (want \"%s\")\n", what, got, want, err, word ? word : "");
        ++failures;
    }
}

static pww_concat_gn_desc_t gn(int C1, int C2, int HW, int G) {
    pww_concat_gn_desc_t d;
    memset(&d, 0, sizeof d);
    d.size = sizeof d; d.dtype = PWW_DTYPE_BF16; d.B = 2; d.C1 = C1; d.C2 = C2; d.HW = HW; d.G = G; d.eps = 1e-5f; d.act = PWW_ACT_SILU;
    return d;
}

static pww_concat_tail_desc_t tail(int Cin, int C1, int C2, int Cout, int splitk) {
    pww_concat_tail_desc_t d;
    memset(&d, 0, sizeof d);
    d.size = sizeof d; d.dtype = PWW_DTYPE_F16; d.B = 2; d.H = 8; d.W = 8; d.Cin = Cin; d.C1 = C1; d.C2 = C2; d.Cout = Cout; d.splitk = splitk;
    return d;
}

int main() {
    alignas(16) static char buf[64];
    void *p = buf, *odd = buf + 8;

    if (pww_concat_version() != PWW_CONCAT_VERSION) { printf("FAIL version\n"); ++failures; }

    // ---- GroupNorm
    pww_concat_gn_desc_t g = gn(64, 32, 64, 8);
    if (pww_concat_group_norm_workspace_bytes(&g) != 16) { printf("FAIL gn workspace (single launch)\n"); ++failures; }
    g = gn(64, 32, 2304, 8);
    if (pww_concat_group_norm_workspace_bytes(&g) != (size_t)2 * 14 * 8 * 16) { printf("FAIL gn workspace (two launches): %zu\n", pww_concat_group_norm_workspace_bytes(&g)); ++failures; }
    const int bad_gn[][4] = {{60, 36, 64, 8}, {64, 36, 64, 4}, {0, 96, 64, 8}, {64, 32, 35, 8}, {64, 32, 4, 8}, {64, 32, 64, 7}, {64, 32, 64, 48}, {2048, 2056, 64, 8}};
    for (const auto &b : bad_gn) {
        g = gn(b[0], b[1], b[2], b[3]);
        expect(pww_concat_group_norm_fwd(p, p, p, p, p, &g, p, 1 << 20, nullptr), PWW_ENOTSUP, "unsupported", "gn shape");
        if (pww_concat_group_norm_workspace_bytes(&g) != 0) { printf("FAIL gn workspace of a bad shape\n"); ++failures; }
    }
    g = gn(64, 32, 64, 8); g.dtype = 2;
    expect(pww_concat_group_norm_fwd(p, p, p, p, p, &g, p, 16, nullptr), PWW_ENOTSUP, "dtype 2", "gn dtype");
    g = gn(64, 32, 64, 8); g.act = 5;
    expect(pww_concat_group_norm_fwd(p, p, p, p, p, &g, p, 16, nullptr), PWW_ENOTSUP, "act 5", "gn act");
    g = gn(64, 32, 64, 8); g.size = 8;
    expect(pww_concat_group_norm_fwd(p, p, p, p, p, &g, p, 16, nullptr), PWW_EINVAL, "older", "gn short descriptor");
    expect(pww_concat_group_norm_fwd(p, p, p, p, p, nullptr, p, 16, nullptr), PWW_EINVAL, "missing", "gn null descriptor");
    g = gn(64, 32, 64, 8);
    expect(pww_concat_group_norm_fwd(nullptr, p, p, p, p, &g, p, 16, nullptr), PWW_EINVAL, "required", "gn x1 null");
    expect(pww_concat_group_norm_fwd(p, nullptr, p, p, p, &g, p, 16, nullptr), PWW_EINVAL, "required", "gn x2 null");
    expect(pww_concat_group_norm_fwd(p, p, p, p, nullptr, &g, p, 16, nullptr), PWW_EINVAL, "required", "gn y null");
    expect(pww_concat_group_norm_fwd(p, p, p, p, p, &g, nullptr, 16, nullptr), PWW_EINVAL, "required", "gn workspace null");
    expect(pww_concat_group_norm_fwd(odd, p, p, p, p, &g, p, 16, nullptr), PWW_EINVAL, "aligned", "gn x1 misaligned");
    expect(pww_concat_group_norm_fwd(p, odd, p, p, p, &g, p, 16, nullptr), PWW_EINVAL, "aligned", "gn x2 misaligned");
    expect(pww_concat_group_norm_fwd(p, p, odd, p, p, &g, p, 16, nullptr), PWW_EINVAL, "aligned", "gn gamma misaligned");
    expect(pww_concat_group_norm_fwd(p, p, p, odd, p, &g, p, 16, nullptr), PWW_EINVAL, "aligned", "gn beta misaligned");
    expect(pww_concat_group_norm_fwd(p, p, p, p, odd, &g, p, 16, nullptr), PWW_EINVAL, "aligned", "gn y misaligned");
    expect(pww_concat_group_norm_fwd(p, p, p, p, p, &g, p, 15, nullptr), PWW_EINVAL, "workspace", "gn workspace short");

    // ---- conv2 + shortcut
    pww_concat_tail_desc_t t = tail(64, 64, 128, 64, 5);
    if (pww_concat_convtail_workspace_bytes(&t) != (size_t)5 * 128 * 64 * 4) { printf("FAIL tail workspace\n"); ++failures; }
    t = tail(64, 64, 128, 64, 1);
    if (pww_concat_convtail_workspace_bytes(&t) != 0) { printf("FAIL tail workspace (unsplit)\n"); ++failures; }
    const int bad_tail[][4] = {{96, 64, 64, 64}, {64, 32, 96, 64}, {64, 64, 96, 64}, {64, 0, 128, 64}, {64, 64, 64, 72}};
    for (const auto &b : bad_tail) {
        t = tail(b[0], b[1], b[2], b[3], 1);
        expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, nullptr, 0, nullptr), PWW_ENOTSUP, "multiples of 64", "tail shape");
        if (pww_concat_convtail_workspace_bytes(&t) != 0) { printf("FAIL tail workspace of a bad shape\n"); ++failures; }
    }
    t = tail(64, 64, 64, 64, 1); t.dtype = 3;
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, nullptr, 0, nullptr), PWW_ENOTSUP, "dtype 3", "tail dtype");
    t = tail(64, 64, 64, 64, 1); t.B = 4096; t.H = 64; t.W = 64;
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, nullptr, 0, nullptr), PWW_ENOTSUP, "2^31", "tail size");
    t = tail(64, 64, 64, 64, 12);
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, p, 1 << 30, nullptr), PWW_ENOTSUP, "exceeds the 11 K-slabs", "tail split");
    t = tail(64, 64, 64, 64, 1); t.tile_n = 128;
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, nullptr, 0, nullptr), PWW_ENOTSUP, "tile_n 128", "tail tile");
    t = tail(64, 64, 64, 64, 1); t.size = 12;
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, nullptr, 0, nullptr), PWW_EINVAL, "older", "tail short descriptor");
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, nullptr, nullptr, 0, nullptr), PWW_EINVAL, "missing", "tail null descriptor");
    t = tail(64, 64, 128, 64, 1);
    for (int k = 0; k < 8; ++k) {
        void *a[8] = {p, p, p, p, p, p, p, p};
        a[k] = nullptr;
        expect(pww_concat_convtail_fwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], &t, nullptr, 0, nullptr), PWW_EINVAL, "required", "tail null pointer");
        a[k] = (k == 5 || k == 6) ? (void *)(buf + 4) : odd;           // the biases: 8-byte alignment
        expect(pww_concat_convtail_fwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], &t, nullptr, 0, nullptr), PWW_EINVAL, "aligned", "tail misaligned pointer");
    }
    t = tail(64, 64, 128, 64, 4);
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, nullptr, 0, nullptr), PWW_EINVAL, "workspace", "tail workspace null");
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, p, 64, nullptr), PWW_EINVAL, "workspace", "tail workspace short");
    expect(pww_concat_convtail_fwd(p, p, p, p, p, p, p, p, &t, odd, 1 << 30, nullptr), PWW_EINVAL, "workspace", "tail workspace misaligned");

    if (failures) { printf("concat_host_check: %d failure(s)\n", failures); return 1; }
    printf("concat_host_check OK\n");
    return 0;
}
