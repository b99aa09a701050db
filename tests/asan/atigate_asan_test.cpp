// Host-side sanitizer test of the GMTI ATI gate's entry points (include/sarx_atigate.h; `make asan-atigate` in csrc/,
// tests/test_atigate.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check and the size query,
// which need no device, are called with valid parameters and with every kind of bad one (looks outside the guard box, an empty
// training set, guard + train of 33, unknown flag bits, NaN, capacities 0 and 16385, NULL), and the launch entry point with the
// arguments a careless caller would pass (NULL context, NULL parameters or buffers, misaligned or overlapping buffers, bad image
// sizes, statistics left out).  Every call must return an error code with a message - never crash.  Exit code 0 and no sanitizer
// report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/sarx_atigate.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_atigate_params good() {
    sarx_atigate_params p{};
    p.guard_az = 2; p.guard_rg = 2; p.train_az = 8; p.train_rg = 8; p.look_az = 1; p.look_rg = 1;
    p.k_sigma = 3.0; p.phase_min = 0.0; p.min_coh = 0.3; p.min_train = 208; p.max_detections = 8;
    p.flags = SARX_ATIGATE_KEEP_UNTESTED;
    return p;
}

static void parameter_check() {
    CHECK(sizeof(sarx_atigate_params) == 64 && sizeof(sarx_atigate_stat) == 96);
    sarx_atigate_params p = good();
    CHECK(sarx_atigate_check(&p) == SARX_OK);
    p.guard_az = 4; p.guard_rg = 2; p.train_az = 28; p.train_rg = 30; p.look_az = 4; p.look_rg = 2;      // outer half-width 32: the limit
    p.phase_min = 3.14159265358979323846; p.min_coh = 1.0; p.k_sigma = 1e300; p.max_detections = SARX_ATIGATE_MAX_DETECTIONS;
    p.min_train = 1 << 30; p.flags = 0;
    CHECK(sarx_atigate_check(&p) == SARX_OK);
    p = good();
    p.guard_az = p.guard_rg = 0; p.train_az = 0; p.train_rg = 1; p.look_az = p.look_rg = 0; p.k_sigma = 0.0; p.min_coh = 0.0;
    p.min_train = 1; p.max_detections = 1;
    CHECK(sarx_atigate_check(&p) == SARX_OK);
    CHECK(sarx_atigate_check(nullptr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    struct { const char* what; void (*edit)(sarx_atigate_params&, double, double); } bad[] = {
        {"guard negative", [](sarx_atigate_params& q, double, double) { q.guard_az = -1; }},
        {"train negative", [](sarx_atigate_params& q, double, double) { q.train_rg = -1; }},
        {"guard + train 33 az", [](sarx_atigate_params& q, double, double) { q.guard_az = 4; q.train_az = 29; }},
        {"guard + train 33 rg", [](sarx_atigate_params& q, double, double) { q.guard_rg = 3; q.train_rg = 30; }},
        {"guard + train wraps", [](sarx_atigate_params& q, double, double) { q.guard_az = INT32_MAX; q.train_az = INT32_MAX; }},
        {"empty training set", [](sarx_atigate_params& q, double, double) { q.train_az = q.train_rg = 0; }},
        {"look az outside guard", [](sarx_atigate_params& q, double, double) { q.look_az = 3; }},
        {"look rg outside guard", [](sarx_atigate_params& q, double, double) { q.look_rg = 3; }},
        {"look 5", [](sarx_atigate_params& q, double, double) { q.guard_az = 6; q.look_az = 5; }},
        {"look negative", [](sarx_atigate_params& q, double, double) { q.look_rg = -1; }},
        {"k_sigma NaN", [](sarx_atigate_params& q, double n, double) { q.k_sigma = n; }},
        {"k_sigma inf", [](sarx_atigate_params& q, double, double i) { q.k_sigma = i; }},
        {"k_sigma negative", [](sarx_atigate_params& q, double, double) { q.k_sigma = -1.0; }},
        {"phase_min NaN", [](sarx_atigate_params& q, double n, double) { q.phase_min = n; }},
        {"phase_min negative", [](sarx_atigate_params& q, double, double) { q.phase_min = -0.1; }},
        {"phase_min past pi", [](sarx_atigate_params& q, double, double) { q.phase_min = 3.2; }},
        {"min_coh NaN", [](sarx_atigate_params& q, double n, double) { q.min_coh = n; }},
        {"min_coh 1.5", [](sarx_atigate_params& q, double, double) { q.min_coh = 1.5; }},
        {"min_coh negative", [](sarx_atigate_params& q, double, double) { q.min_coh = -0.5; }},
        {"min_train 0", [](sarx_atigate_params& q, double, double) { q.min_train = 0; }},
        {"capacity 0", [](sarx_atigate_params& q, double, double) { q.max_detections = 0; }},
        {"capacity negative", [](sarx_atigate_params& q, double, double) { q.max_detections = -1; }},
        {"capacity 16385", [](sarx_atigate_params& q, double, double) { q.max_detections = SARX_ATIGATE_MAX_DETECTIONS + 1; }},
        {"unknown flag", [](sarx_atigate_params& q, double, double) { q.flags = 2u; }},
        {"unknown high flag", [](sarx_atigate_params& q, double, double) { q.flags = 0x80000001u; }},
        {"reserved set", [](sarx_atigate_params& q, double, double) { q.reserved = 1u; }},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p, nan, inf);
        size_t n = 12345;
        int rc = sarx_atigate_check(&p);
        if (rc != SARX_ERR_INVALID) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
        rc = sarx_atigate_stats_bytes(&p, &n);
        if (rc != SARX_ERR_INVALID || n != 12345) { ++failures; fprintf(stderr, "FAIL stats_bytes %s: rc %d\n", b.what, rc); }
        alignas(16) static char buf[4096];
        CHECK(sarx_atigate_step_dev(nullptr, &p, buf, buf + 512, 4, 4, buf + 1024, buf + 2048, nullptr) != SARX_OK);
    }
}

static void sizes() {
    sarx_atigate_params p = good();
    size_t n = 0;
    CHECK(sarx_atigate_stats_bytes(&p, &n) == SARX_OK && n == 96 * 8);
    p.max_detections = SARX_ATIGATE_MAX_DETECTIONS;
    CHECK(sarx_atigate_stats_bytes(&p, &n) == SARX_OK && n == (size_t)96 * 16384);
    CHECK(sarx_atigate_stats_bytes(&p, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_atigate_stats_bytes(nullptr, &n) == SARX_ERR_INVALID);
}

static void launch_without_a_context() {
    sarx_atigate_params p = good();                  // slot: 16 + 48 * 8 = 400 bytes, statistics 768, a 4 x 4 image 128
    alignas(16) static char buf[8192];
    char* a = buf; char* b = buf + 512; char* in = buf + 1024; char* out = buf + 2048; char* stats = buf + 4096;
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, out, stats) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, out, nullptr) != SARX_OK);                  // statistics left out
    CHECK(sarx_atigate_step_dev(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, nullptr, b, 4, 4, in, out, stats) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, nullptr, 4, 4, in, out, stats) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, nullptr, out, stats) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, nullptr, stats) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 0, 4, in, out, stats) != SARX_OK);                    // image sizes
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, -1, in, out, stats) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, INT32_MAX, INT32_MAX, in, out, stats) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a + 4, b, 4, 4, in, out, stats) != SARX_OK);                // misaligned
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in + 4, out, stats) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, out + 2, stats + 4) != SARX_OK);
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, in, stats) != SARX_OK);                     // in place
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, in + 392, stats) != SARX_OK);               // the last 8 bytes shared
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, a + 120, stats) != SARX_OK);                // output over an image
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, out, out + 16) != SARX_OK);                 // statistics over the output
    CHECK(sarx_atigate_step_dev(nullptr, &p, a, b, 4, 4, in, out, b) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    sizes();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "atigate_asan_test: %d failures\n", failures); return 1; }
    printf("atigate_asan_test: all checks passed\n");
    return 0;
}
