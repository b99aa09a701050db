// Host-side sanitizer test of the GMTI entry points (include/sarx_gmti.h; `make asan-gmti` in csrc/, tests/test_gmti.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp (every translation unit with -fsanitize=address,undefined for the
// HOST pass).  Runs where there is no GPU: every entry point of the header is called with the arguments a careless caller would
// pass (NULL context, NULL parameters, NULL or misaligned buffers, bad sizes, half-widths out of range, alpha <= 0 or NaN, an empty
// training set, no report capacity) and must return an error code with a message - never crash.  The slot size query, which needs
// no device, is also checked on valid parameters.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_gmti.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_gmti_params good() {
    sarx_gmti_params p{};
    p.guard_az = 2; p.guard_rg = 2; p.train_az = 8; p.train_rg = 8;
    p.alpha = 10.0; p.min_train = 200; p.max_detections = 4096;
    return p;
}

static void slot_query() {
    size_t n = 0;
    sarx_gmti_params p = good();
    CHECK(sizeof(sarx_gmti_header) == 16 && sizeof(sarx_gmti_report) == 48);
    CHECK(sarx_gmti_slot_bytes(&p, &n) == SARX_OK && n == 16 + 48 * (size_t)4096);
    p.guard_az = 0; p.guard_rg = 0; p.train_az = SARX_GMTI_MAX_HALF; p.train_rg = 0; p.max_detections = 1;
    CHECK(sarx_gmti_slot_bytes(&p, &n) == SARX_OK && n == 64);          // the limit itself is allowed
    CHECK(sarx_gmti_slot_bytes(nullptr, &n) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    p = good();
    CHECK(sarx_gmti_slot_bytes(&p, nullptr) == SARX_ERR_INVALID);
    struct { const char* what; void (*edit)(sarx_gmti_params&); int code; } bad[] = {
        {"negative guard", [](sarx_gmti_params& q) { q.guard_az = -1; }, SARX_ERR_INVALID},
        {"negative train", [](sarx_gmti_params& q) { q.train_rg = -3; }, SARX_ERR_INVALID},
        {"azimuth halo", [](sarx_gmti_params& q) { q.guard_az = 2; q.train_az = 31; }, SARX_ERR_UNSUPPORTED},
        {"range halo", [](sarx_gmti_params& q) { q.guard_rg = 33; q.train_rg = 0; }, SARX_ERR_UNSUPPORTED},
        {"empty training set", [](sarx_gmti_params& q) { q.train_az = 0; q.train_rg = 0; }, SARX_ERR_INVALID},
        {"alpha 0", [](sarx_gmti_params& q) { q.alpha = 0.0; }, SARX_ERR_INVALID},
        {"alpha < 0", [](sarx_gmti_params& q) { q.alpha = -2.0; }, SARX_ERR_INVALID},
        {"alpha NaN", [](sarx_gmti_params& q) { q.alpha = std::nan(""); }, SARX_ERR_INVALID},
        {"alpha inf", [](sarx_gmti_params& q) { q.alpha = INFINITY; }, SARX_ERR_INVALID},
        {"min_train 0", [](sarx_gmti_params& q) { q.min_train = 0; }, SARX_ERR_INVALID},
        {"no capacity", [](sarx_gmti_params& q) { q.max_detections = 0; }, SARX_ERR_INVALID},
        {"negative capacity", [](sarx_gmti_params& q) { q.max_detections = -5; }, SARX_ERR_INVALID},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        n = 12345;
        const int rc = sarx_gmti_slot_bytes(&p, &n);
        if (rc != b.code) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(n == 12345);                                                  // nothing written on failure
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
    }
}

static void launches_without_a_context() {
    sarx_gmti_params p = good();
    alignas(16) static char buf[4096];
    float* mag = (float*)buf;
    sarx_gmti_report* rep = (sarx_gmti_report*)(buf + 64);
    sarx_gmti_header* hdr = (sarx_gmti_header*)buf;
    CHECK(sarx_gmti_cfar_dev(nullptr, mag, 64, 64, &p, rep, hdr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_gmti_cfar_dev(nullptr, nullptr, 0, -1, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_gmti_cfar_dev(nullptr, mag, 64, 64, &p, (sarx_gmti_report*)(buf + 3), hdr) != SARX_OK);
    CHECK(sarx_gmti_refine_dev(nullptr, buf, buf, 64, 64, 0.0, rep, hdr, 16) == SARX_ERR_INVALID);
    CHECK(sarx_gmti_refine_dev(nullptr, nullptr, nullptr, 0, 0, NAN, nullptr, nullptr, 0) != SARX_OK);
    CHECK(sarx_gmti_refine_dev(nullptr, buf, buf, 64, 64, 0.0, rep, hdr, -1) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    slot_query();
    launches_without_a_context();
    if (failures) { fprintf(stderr, "gmti_asan_test: %d failures\n", failures); return 1; }
    printf("gmti_asan_test: all checks passed\n");
    return 0;
}
