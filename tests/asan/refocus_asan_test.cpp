// Host-side sanitizer test of the GMTI refocus entry points (include/sarx_refocus.h; `make asan-refocus` in csrc/,
// tests/test_refocus.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check, which needs no
// device, is called with valid parameters and with every kind of bad one (chip length and width, source, hypothesis count and
// speeds, radar constants, L > n_az, NULL), and the launch entry point with the arguments a careless caller would pass (NULL
// context, NULL parameters or buffers, misaligned buffers, no capacity).  Every call must return an error code with a message -
// never crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_refocus.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_refocus_params good() {
    sarx_refocus_params p{};
    p.chip_az = 256; p.chip_rg = 5; p.source = SARX_REFOCUS_DPCA; p.n_hyp = 33;
    p.wavelength_m = 0.031; p.platform_speed_mps = 7500.0; p.prf_hz = 6000.0; p.r0_m = 8.4e5; p.dr_m = 0.25; p.cal_phase = 0.1;
    for (int k = 0; k < SARX_REFOCUS_MAX_HYP; ++k) p.speed_mps[k] = 7500.0 * (1.0 - (k - 16) * 2.5 / 7300.0);
    return p;
}

static void parameter_check() {
    CHECK(sizeof(sarx_refocus_params) == 576 && sizeof(sarx_refocus_record) == 48);
    sarx_refocus_params p = good();
    CHECK(sarx_refocus_check(&p, 8192, 8192) == SARX_OK);
    p.chip_az = 512; p.chip_rg = SARX_REFOCUS_MAX_W; p.n_hyp = SARX_REFOCUS_MAX_HYP; p.source = SARX_REFOCUS_SLC1;
    CHECK(sarx_refocus_check(&p, 512, 1) == SARX_OK);                        // the limits themselves are allowed
    p = good();
    p.chip_az = 64; p.chip_rg = 1; p.n_hyp = 1;
    CHECK(sarx_refocus_check(&p, 64, 1) == SARX_OK);
    CHECK(sarx_refocus_check(nullptr, 1024, 1024) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* what; void (*edit)(sarx_refocus_params&); int n_az, n_rg, code; } bad[] = {
        {"L 32", [](sarx_refocus_params& q) { q.chip_az = 32; }, 1024, 64, SARX_ERR_UNSUPPORTED},
        {"L 1024", [](sarx_refocus_params& q) { q.chip_az = 1024; }, 4096, 64, SARX_ERR_UNSUPPORTED},
        {"L 200", [](sarx_refocus_params& q) { q.chip_az = 200; }, 1024, 64, SARX_ERR_UNSUPPORTED},
        {"L > n_az", [](sarx_refocus_params& q) { q.chip_az = 512; }, 511, 64, SARX_ERR_INVALID},
        {"W even", [](sarx_refocus_params& q) { q.chip_rg = 4; }, 1024, 64, SARX_ERR_INVALID},
        {"W 0", [](sarx_refocus_params& q) { q.chip_rg = 0; }, 1024, 64, SARX_ERR_INVALID},
        {"W 17", [](sarx_refocus_params& q) { q.chip_rg = 17; }, 1024, 64, SARX_ERR_INVALID},
        {"W negative", [](sarx_refocus_params& q) { q.chip_rg = -3; }, 1024, 64, SARX_ERR_INVALID},
        {"source", [](sarx_refocus_params& q) { q.source = 2; }, 1024, 64, SARX_ERR_INVALID},
        {"n_hyp 0", [](sarx_refocus_params& q) { q.n_hyp = 0; }, 1024, 64, SARX_ERR_INVALID},
        {"n_hyp 65", [](sarx_refocus_params& q) { q.n_hyp = SARX_REFOCUS_MAX_HYP + 1; }, 1024, 64, SARX_ERR_INVALID},
        {"lambda 0", [](sarx_refocus_params& q) { q.wavelength_m = 0.0; }, 1024, 64, SARX_ERR_INVALID},
        {"V_r NaN", [](sarx_refocus_params& q) { q.platform_speed_mps = std::nan(""); }, 1024, 64, SARX_ERR_INVALID},
        {"prf < 0", [](sarx_refocus_params& q) { q.prf_hz = -1.0; }, 1024, 64, SARX_ERR_INVALID},
        {"r0 inf", [](sarx_refocus_params& q) { q.r0_m = INFINITY; }, 1024, 64, SARX_ERR_INVALID},
        {"dr NaN", [](sarx_refocus_params& q) { q.dr_m = std::nan(""); }, 1024, 64, SARX_ERR_INVALID},
        {"cal inf", [](sarx_refocus_params& q) { q.cal_phase = -INFINITY; }, 1024, 64, SARX_ERR_INVALID},
        {"speed 0", [](sarx_refocus_params& q) { q.speed_mps[32] = 0.0; }, 1024, 64, SARX_ERR_INVALID},
        {"speed NaN", [](sarx_refocus_params& q) { q.speed_mps[0] = std::nan(""); }, 1024, 64, SARX_ERR_INVALID},
        {"image 0 rows", [](sarx_refocus_params&) {}, 0, 64, SARX_ERR_INVALID},
        {"image -1 cols", [](sarx_refocus_params&) {}, 1024, -1, SARX_ERR_INVALID},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        const int rc = sarx_refocus_check(&p, b.n_az, b.n_rg);
        if (rc != b.code) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
    }
    p = good();
    p.n_hyp = 3;
    p.speed_mps[40] = std::nan("");                                          // past n_hyp: not looked at
    CHECK(sarx_refocus_check(&p, 1024, 64) == SARX_OK);
}

static void launch_without_a_context() {
    sarx_refocus_params p = good();
    alignas(16) static char buf[4096];
    const sarx_gmti_header* hdr = (const sarx_gmti_header*)buf;
    const sarx_gmti_report* rep = (const sarx_gmti_report*)(buf + 16);
    sarx_refocus_record* rec = (sarx_refocus_record*)(buf + 1024);
    float* curves = (float*)(buf + 2048);
    CHECK(sarx_refocus_dev(nullptr, buf, buf, 1024, 64, &p, rep, hdr, 16, rec, curves, buf) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_refocus_dev(nullptr, nullptr, nullptr, 0, -1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_refocus_dev(nullptr, buf, nullptr, 1024, 64, &p, rep, hdr, 16, rec, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_refocus_dev(nullptr, buf + 3, buf, 1024, 64, &p, rep, hdr, 16, rec, curves, nullptr) != SARX_OK);
    CHECK(sarx_refocus_dev(nullptr, buf, buf, 1024, 64, &p, rep, hdr, -1, rec, curves, nullptr) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "refocus_asan_test: %d failures\n", failures); return 1; }
    printf("refocus_asan_test: all checks passed\n");
    return 0;
}
