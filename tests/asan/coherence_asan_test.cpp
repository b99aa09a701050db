// Host-side sanitizer test of the sliding-window coherence entry points (include/sarx_coherence.h; `make asan-coherence` in csrc/,
// tests/test_coherence.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check and the size
// query, which need no device, are called with valid parameters and with every kind of bad one (half-widths, flags, reserved,
// threshold, power floor, image size, NULL), and the two launch entry points with the arguments a careless caller would pass (NULL
// context, NULL parameters or buffers, misaligned and overlapping buffers, bad lags and strides).  Every call must return an error
// code with a message - never crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_coherence.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_coherence_params good() {
    sarx_coherence_params p{};
    p.ha = 4; p.hr = 4; p.flags = 0; p.reserved = 0; p.threshold = 0.5; p.power_floor = 0.0;
    return p;
}

static void parameter_check() {
    CHECK(sizeof(sarx_coherence_params) == 32 && sizeof(sarx_coherence_summary) == 64);
    sarx_coherence_params p = good();
    CHECK(sarx_coherence_check(&p, 8192, 8192) == SARX_OK);
    p.ha = p.hr = SARX_COH_MAX_HALF; p.threshold = 0.0; p.power_floor = 1e300;
    CHECK(sarx_coherence_check(&p, 1 << 20, 1) == SARX_OK);                  // the limits themselves are allowed
    CHECK(sarx_coherence_check(&p, 1, 1) == SARX_OK);                        // a window larger than the image
    p.ha = p.hr = 0;
    CHECK(sarx_coherence_check(&p, 5, 7) == SARX_OK);
    CHECK(sarx_coherence_check(nullptr, 1024, 1024) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* what; void (*edit)(sarx_coherence_params&); int n_az, n_rg, code; } bad[] = {
        {"ha 17", [](sarx_coherence_params& q) { q.ha = 17; }, 1024, 64, SARX_ERR_INVALID},
        {"hr 17", [](sarx_coherence_params& q) { q.hr = 17; }, 1024, 64, SARX_ERR_INVALID},
        {"ha negative", [](sarx_coherence_params& q) { q.ha = -1; }, 1024, 64, SARX_ERR_INVALID},
        {"hr negative", [](sarx_coherence_params& q) { q.hr = INT32_MIN; }, 1024, 64, SARX_ERR_INVALID},
        {"flags", [](sarx_coherence_params& q) { q.flags = 4; }, 1024, 64, SARX_ERR_INVALID},
        {"reserved", [](sarx_coherence_params& q) { q.reserved = 1; }, 1024, 64, SARX_ERR_INVALID},
        {"threshold NaN", [](sarx_coherence_params& q) { q.threshold = std::nan(""); }, 1024, 64, SARX_ERR_INVALID},
        {"threshold inf", [](sarx_coherence_params& q) { q.threshold = INFINITY; }, 1024, 64, SARX_ERR_INVALID},
        {"threshold negative", [](sarx_coherence_params& q) { q.threshold = -1e-9; }, 1024, 64, SARX_ERR_INVALID},
        {"floor NaN", [](sarx_coherence_params& q) { q.power_floor = std::nan(""); }, 1024, 64, SARX_ERR_INVALID},
        {"floor inf", [](sarx_coherence_params& q) { q.power_floor = INFINITY; }, 1024, 64, SARX_ERR_INVALID},
        {"floor negative", [](sarx_coherence_params& q) { q.power_floor = -1.0; }, 1024, 64, SARX_ERR_INVALID},
        {"image 0 rows", [](sarx_coherence_params&) {}, 0, 64, SARX_ERR_INVALID},
        {"image -1 cols", [](sarx_coherence_params&) {}, 1024, -1, SARX_ERR_INVALID},
        {"image too tall", [](sarx_coherence_params&) {}, (1 << 20) + 1, 64, SARX_ERR_UNSUPPORTED},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        size_t n = 12345;
        int rc = sarx_coherence_check(&p, b.n_az, b.n_rg);
        if (rc != b.code) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
        rc = sarx_coherence_workspace_bytes(&p, b.n_az, b.n_rg, &n);
        if (rc != b.code || n != 12345) { ++failures; fprintf(stderr, "FAIL workspace_bytes %s: rc %d\n", b.what, rc); }
    }
}

static void sizes() {
    sarx_coherence_params p = good();
    size_t n = 0, m = 0;
    CHECK(sarx_coherence_workspace_bytes(&p, 1, 1, &n) == SARX_OK && n > 0 && n % 8 == 0);
    CHECK(sarx_coherence_workspace_bytes(&p, 1000, 777, &m) == SARX_OK && m > n && m % 8 == 0);
    CHECK(sarx_coherence_workspace_bytes(&p, 64, 64, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_coherence_workspace_bytes(nullptr, 64, 64, &n) == SARX_ERR_INVALID);
}

static void launch_without_a_context() {
    sarx_coherence_params p = good();
    alignas(16) static char buf[8192];
    float* coh = (float*)(buf + 4096);
    CHECK(sarx_coherence_pair_dev(nullptr, buf, buf + 1024, 8, 8, &p, coh, nullptr, nullptr, nullptr, nullptr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_coherence_pair_dev(nullptr, nullptr, nullptr, 0, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_coherence_pair_dev(nullptr, buf + 4, buf, 8, 8, &p, coh, nullptr, nullptr, nullptr, nullptr) != SARX_OK);            // misaligned
    CHECK(sarx_coherence_pair_dev(nullptr, buf, buf, 8, 8, &p, (float*)buf, nullptr, nullptr, nullptr, nullptr) != SARX_OK);        // aliased
    CHECK(sarx_coherence_pair_dev(nullptr, buf, buf, 8, 8, &p, coh, nullptr, nullptr, buf + 6144, nullptr) != SARX_OK);            // summary, no workspace
    CHECK(sarx_coherence_stack_dev(nullptr, buf, 3, 512, 1, 8, 8, &p, coh, 256, nullptr, 0, nullptr, 0, nullptr, nullptr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_coherence_stack_dev(nullptr, buf, 3, 512, 3, 8, 8, &p, coh, 256, nullptr, 0, nullptr, 0, nullptr, nullptr) != SARX_OK);   // lag >= n_frames
    CHECK(sarx_coherence_stack_dev(nullptr, buf, 3, 100, 1, 8, 8, &p, coh, 256, nullptr, 0, nullptr, 0, nullptr, nullptr) != SARX_OK);   // stride too small
    CHECK(sarx_coherence_stack_dev(nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    sizes();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "coherence_asan_test: %d failures\n", failures); return 1; }
    printf("coherence_asan_test: all checks passed\n");
    return 0;
}
