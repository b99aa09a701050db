// Host-side sanitizer test of the phase-gradient autofocus entry points (include/sarx_pga.h; `make asan-pga` in csrc/,
// tests/test_pga.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check and the size
// query, which need no device, are called with valid parameters and with every kind of bad one (azimuth length, half-widths,
// iteration count, leading dimension, overlapping frames, contrast, floor, NULL), and the two launch entry points with the
// arguments a careless caller would pass (NULL context, NULL parameters or buffers, overlapping buffers, bad signs and strides).
// Every call must return an error code with a message - never crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_pga.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_pga_params good() {
    sarx_pga_params p{};
    p.n_iter = 4;
    p.half_width[0] = 64; p.half_width[1] = 32; p.half_width[2] = 16; p.half_width[3] = 8;
    p.min_contrast = 3.0;
    p.power_floor = 0.05;
    return p;
}

struct Layout { int n_az, n_rg; size_t ld; int n_frames; size_t stride; };
static const Layout FRAME = {256, 100, 100, 1, 0};

static void parameter_check() {
    CHECK(sizeof(sarx_pga_params) == 56 && sizeof(sarx_pga_record) == 32);
    sarx_pga_params p = good();
    CHECK(sarx_pga_check(&p, 256, 100, 100, 1, 0) == SARX_OK);
    CHECK(sarx_pga_check(&p, 512, 512, 512, 46, (size_t)512 * 512) == SARX_OK);
    CHECK(sarx_pga_check(&p, 1024, 1, 7, 3, (size_t)1023 * 7 + 1) == SARX_OK);             // frames that just touch
    CHECK(sarx_pga_check(&p, 256, SARX_PGA_MAX_RG, SARX_PGA_MAX_RG, 1, 0) == SARX_OK);      // the limits themselves are allowed
    p.n_iter = SARX_PGA_MAX_ITER;
    for (int i = 0; i < SARX_PGA_MAX_ITER; ++i) p.half_width[i] = 31;
    p.min_contrast = 0.0; p.power_floor = 0.0;
    CHECK(sarx_pga_check(&p, 64, 5, 9, SARX_PGA_MAX_FRAMES, 64 * 9) == SARX_OK);
    CHECK(sarx_pga_check(nullptr, 256, 100, 100, 1, 0) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* what; void (*edit)(sarx_pga_params&); Layout g; } bad[] = {
        {"L 100", [](sarx_pga_params&) {}, {100, 100, 100, 1, 0}},
        {"L 2048", [](sarx_pga_params&) {}, {2048, 100, 100, 1, 0}},
        {"L negative", [](sarx_pga_params&) {}, {INT32_MIN, 100, 100, 1, 0}},
        {"2h + 1 > L", [](sarx_pga_params& q) { q.half_width[0] = 128; }, FRAME},
        {"h 0", [](sarx_pga_params& q) { q.half_width[3] = 0; }, FRAME},
        {"h negative", [](sarx_pga_params& q) { q.half_width[1] = INT32_MIN; }, FRAME},
        {"h INT_MAX", [](sarx_pga_params& q) { q.half_width[2] = INT32_MAX; }, FRAME},
        {"n_iter 0", [](sarx_pga_params& q) { q.n_iter = 0; }, FRAME},
        {"n_iter 9", [](sarx_pga_params& q) { q.n_iter = 9; }, FRAME},
        {"n_iter negative", [](sarx_pga_params& q) { q.n_iter = INT32_MIN; }, FRAME},
        {"reserved", [](sarx_pga_params& q) { q.reserved = 1; }, FRAME},
        {"contrast negative", [](sarx_pga_params& q) { q.min_contrast = -1e-9; }, FRAME},
        {"contrast NaN", [](sarx_pga_params& q) { q.min_contrast = std::nan(""); }, FRAME},
        {"contrast inf", [](sarx_pga_params& q) { q.min_contrast = INFINITY; }, FRAME},
        {"floor 1", [](sarx_pga_params& q) { q.power_floor = 1.0; }, FRAME},
        {"floor negative", [](sarx_pga_params& q) { q.power_floor = -0.5; }, FRAME},
        {"floor NaN", [](sarx_pga_params& q) { q.power_floor = std::nan(""); }, FRAME},
        {"n_rg 0", [](sarx_pga_params&) {}, {256, 0, 100, 1, 0}},
        {"n_rg too large", [](sarx_pga_params&) {}, {256, SARX_PGA_MAX_RG + 1, (size_t)SARX_PGA_MAX_RG + 1, 1, 0}},
        {"ld < n_rg", [](sarx_pga_params&) {}, {256, 100, 99, 1, 0}},
        {"ld huge", [](sarx_pga_params&) {}, {256, 100, SIZE_MAX, 1, 0}},
        {"frames 0", [](sarx_pga_params&) {}, {256, 100, 100, 0, 0}},
        {"frames too many", [](sarx_pga_params&) {}, {256, 100, 100, SARX_PGA_MAX_FRAMES + 1, 25600}},
        {"frames overlap", [](sarx_pga_params&) {}, {256, 100, 100, 2, 255 * 100 + 99}},
        {"stride 0", [](sarx_pga_params&) {}, {256, 100, 100, 2, 0}},
        {"stride huge", [](sarx_pga_params&) {}, {256, 100, 100, 2, SIZE_MAX}},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        size_t n = 12345;
        int rc = sarx_pga_check(&p, b.g.n_az, b.g.n_rg, b.g.ld, b.g.n_frames, b.g.stride);
        if (rc != SARX_ERR_INVALID) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
        rc = sarx_pga_workspace_bytes(&p, b.g.n_az, b.g.n_rg, b.g.ld, b.g.n_frames, b.g.stride, &n);
        if (rc != SARX_ERR_INVALID || n != 12345) { ++failures; fprintf(stderr, "FAIL workspace_bytes %s: rc %d\n", b.what, rc); }
    }
}

static void sizes() {
    sarx_pga_params p = good();
    size_t n = 0, m = 0;
    CHECK(sarx_pga_workspace_bytes(&p, 512, 1, 1, 1, 0, &n) == SARX_OK && n == (3 * 512 + 4) * 8);
    CHECK(sarx_pga_workspace_bytes(&p, 512, 512, 512, 46, (size_t)512 * 512, &m) == SARX_OK && m == n * 64 * 46);
    CHECK(sarx_pga_workspace_bytes(&p, 256, SARX_PGA_MAX_RG, SARX_PGA_MAX_RG, SARX_PGA_MAX_FRAMES, (size_t)256 * SARX_PGA_MAX_RG, &m) == SARX_OK && m > n);
    CHECK(sarx_pga_workspace_bytes(&p, 512, 512, 512, 1, 0, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_pga_workspace_bytes(nullptr, 512, 512, 512, 1, 0, &n) == SARX_ERR_INVALID);
}

static void launch_without_a_context() {
    sarx_pga_params p = good();
    alignas(16) static char buf[16384];
    double* phase = (double*)(buf + 8192);
    sarx_pga_record* rec = (sarx_pga_record*)(buf + 12288);
    CHECK(sarx_pga_dev(nullptr, buf, buf + 4096, 64, 4, 4, 1, 0, &p, phase, rec, buf + 14336) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_pga_dev(nullptr, nullptr, nullptr, 0, -1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_pga_dev(nullptr, buf, buf, 64, 4, 4, 1, 0, &p, phase, rec, buf + 14336) != SARX_OK);                  // in place
    CHECK(sarx_pga_dev(nullptr, buf + 4, buf + 4096, 64, 4, 4, 1, 0, &p, phase, rec, nullptr) != SARX_OK);           // misaligned, no workspace
    CHECK(sarx_pga_apply_dev(nullptr, buf, buf + 4096, 64, 4, 4, 1, 0, phase, 0, -1) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_pga_apply_dev(nullptr, buf, buf + 4096, 64, 4, 4, 1, 0, phase, 0, 0) != SARX_OK);                     // sign 0
    CHECK(sarx_pga_apply_dev(nullptr, buf, buf + 4096, 64, 4, 4, 2, 10, phase, 3, 1) != SARX_OK);                    // strides too small
    CHECK(sarx_pga_apply_dev(nullptr, buf, buf, 64, 4, 4, 1, 0, phase, 0, 1) != SARX_OK);                            // in place
    CHECK(sarx_pga_apply_dev(nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, 0, 0) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    sizes();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "pga_asan_test: %d failures\n", failures); return 1; }
    printf("pga_asan_test: all checks passed\n");
    return 0;
}
