// Host-side sanitizer test of the OS-CFAR entry points (include/sarx_oscfar.h; `make asan-oscfar` in csrc/, tests/test_oscfar.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp (every translation unit with -fsanitize=address,undefined for the
// HOST pass).  Runs where there is no GPU: both entry points of the header are called with the arguments a careless caller would
// pass (NULL context, NULL parameters, NULL or misaligned buffers, bad sizes, every refusal of the CA launch's parameters, a rank
// outside 1 .. N_full, flags) and must return an error code with a message - never crash.  The check, which needs no device, is
// also held to valid parameters.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_oscfar.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_oscfar_params good() {
    sarx_oscfar_params p{};
    p.base.guard_az = 2; p.base.guard_rg = 2; p.base.train_az = 8; p.base.train_rg = 8;      // N_full = 416
    p.base.alpha = 10.0; p.base.min_train = 208; p.base.max_detections = 4096;
    p.rank = 312; p.flags = 0;
    return p;
}

static void check_query() {
    sarx_oscfar_params p = good();
    CHECK(sizeof(sarx_oscfar_params) == 40);
    CHECK(sarx_oscfar_check(&p) == SARX_OK);
    p.rank = 1;
    CHECK(sarx_oscfar_check(&p) == SARX_OK);
    p.rank = 416;
    CHECK(sarx_oscfar_check(&p) == SARX_OK);                              // the limits themselves are allowed
    p = good();
    p.base.guard_az = 0; p.base.guard_rg = 0; p.base.train_az = SARX_GMTI_MAX_HALF; p.base.train_rg = 0; p.rank = 64;
    CHECK(sarx_oscfar_check(&p) == SARX_OK);                              // N_full = 65 - 1
    p.rank = 65;
    CHECK(sarx_oscfar_check(&p) == SARX_ERR_INVALID);
    CHECK(sarx_oscfar_check(nullptr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* what; void (*edit)(sarx_oscfar_params&); int code; } bad[] = {
        {"rank 0", [](sarx_oscfar_params& q) { q.rank = 0; }, SARX_ERR_INVALID},
        {"rank < 0", [](sarx_oscfar_params& q) { q.rank = -7; }, SARX_ERR_INVALID},
        {"rank > N_full", [](sarx_oscfar_params& q) { q.rank = 417; }, SARX_ERR_INVALID},
        {"rank INT_MAX", [](sarx_oscfar_params& q) { q.rank = INT32_MAX; }, SARX_ERR_INVALID},
        {"flags", [](sarx_oscfar_params& q) { q.flags = 1; }, SARX_ERR_INVALID},
        {"negative guard", [](sarx_oscfar_params& q) { q.base.guard_az = -1; }, SARX_ERR_INVALID},
        {"negative train", [](sarx_oscfar_params& q) { q.base.train_rg = -3; }, SARX_ERR_INVALID},
        {"azimuth halo", [](sarx_oscfar_params& q) { q.base.guard_az = 2; q.base.train_az = 31; }, SARX_ERR_UNSUPPORTED},
        {"range halo", [](sarx_oscfar_params& q) { q.base.guard_rg = 33; q.base.train_rg = 0; }, SARX_ERR_UNSUPPORTED},
        {"empty training set", [](sarx_oscfar_params& q) { q.base.train_az = 0; q.base.train_rg = 0; }, SARX_ERR_INVALID},
        {"alpha 0", [](sarx_oscfar_params& q) { q.base.alpha = 0.0; }, SARX_ERR_INVALID},
        {"alpha NaN", [](sarx_oscfar_params& q) { q.base.alpha = std::nan(""); }, SARX_ERR_INVALID},
        {"alpha inf", [](sarx_oscfar_params& q) { q.base.alpha = INFINITY; }, SARX_ERR_INVALID},
        {"min_train 0", [](sarx_oscfar_params& q) { q.base.min_train = 0; }, SARX_ERR_INVALID},
        {"no capacity", [](sarx_oscfar_params& q) { q.base.max_detections = 0; }, SARX_ERR_INVALID},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        const int rc = sarx_oscfar_check(&p);
        if (rc != b.code) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
    }
}

static void launch_without_a_context() {
    sarx_oscfar_params p = good();
    alignas(16) static char buf[4096];
    float* mag = (float*)buf;
    sarx_gmti_report* rep = (sarx_gmti_report*)(buf + 64);
    sarx_gmti_header* hdr = (sarx_gmti_header*)buf;
    CHECK(sarx_gmti_oscfar_dev(nullptr, mag, 64, 64, &p, rep, hdr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_gmti_oscfar_dev(nullptr, nullptr, 0, -1, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_gmti_oscfar_dev(nullptr, mag, 64, 64, &p, (sarx_gmti_report*)(buf + 3), hdr) != SARX_OK);
    p.rank = 0;
    CHECK(sarx_gmti_oscfar_dev(nullptr, mag, 64, 64, &p, rep, hdr) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    check_query();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "oscfar_asan_test: %d failures\n", failures); return 1; }
    printf("oscfar_asan_test: all checks passed\n");
    return 0;
}
