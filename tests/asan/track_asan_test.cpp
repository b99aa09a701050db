// Host-side sanitizer test of the GMTI tracker's entry points (include/sarx_track.h; `make asan-track` in csrc/,
// tests/test_track.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check and the two size
// queries, which need no device, are called with valid parameters and with every kind of bad one (gates, gains, confirmation rule,
// misses, birth ratio, capacities, reserved, NULL), and the three launch entry points with the arguments a careless caller would
// pass (NULL context, NULL parameters or buffers, misaligned buffers, a stride shorter than a slot).  Every call must return an
// error code with a message - never crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_track.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_track_params good() {
    sarx_track_params p{};
    p.gate_az = 4.0; p.gate_rg = 4.0; p.alpha = 0.5; p.beta = 0.25; p.birth_ratio = 0.0;
    p.confirm_hits = 3; p.confirm_window = 5; p.max_misses = 3; p.max_tracks = 1024; p.max_detections = 4096; p.reserved = 0;
    return p;
}

static void parameter_check() {
    CHECK(sizeof(sarx_track_params) == 64 && sizeof(sarx_track_header) == 64 && sizeof(sarx_track_slot) == 96);
    sarx_track_params p = good();
    CHECK(sarx_track_check(&p) == SARX_OK);
    p.alpha = 1.0; p.beta = 2.0; p.confirm_hits = 32; p.confirm_window = 32; p.max_misses = 0; p.max_tracks = SARX_TRACK_MAX_TRACKS;
    p.max_detections = SARX_TRACK_MAX_DETECTIONS; p.gate_az = 1e-300; p.birth_ratio = 1e300;
    CHECK(sarx_track_check(&p) == SARX_OK);                                  // the limits themselves are allowed
    p = good();
    p.confirm_hits = p.confirm_window = 1; p.max_tracks = 1; p.max_detections = 1; p.beta = 0.0;
    CHECK(sarx_track_check(&p) == SARX_OK);
    CHECK(sarx_track_check(nullptr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* what; void (*edit)(sarx_track_params&); } bad[] = {
        {"gate_az 0", [](sarx_track_params& q) { q.gate_az = 0.0; }},
        {"gate_rg negative", [](sarx_track_params& q) { q.gate_rg = -4.0; }},
        {"gate_az NaN", [](sarx_track_params& q) { q.gate_az = std::nan(""); }},
        {"gate_rg inf", [](sarx_track_params& q) { q.gate_rg = INFINITY; }},
        {"alpha 0", [](sarx_track_params& q) { q.alpha = 0.0; }},
        {"alpha 1.5", [](sarx_track_params& q) { q.alpha = 1.5; }},
        {"alpha NaN", [](sarx_track_params& q) { q.alpha = std::nan(""); }},
        {"beta negative", [](sarx_track_params& q) { q.beta = -0.1; }},
        {"beta 2.5", [](sarx_track_params& q) { q.beta = 2.5; }},
        {"beta NaN", [](sarx_track_params& q) { q.beta = std::nan(""); }},
        {"birth negative", [](sarx_track_params& q) { q.birth_ratio = -1.0; }},
        {"birth inf", [](sarx_track_params& q) { q.birth_ratio = INFINITY; }},
        {"hits 0", [](sarx_track_params& q) { q.confirm_hits = 0; }},
        {"hits > window", [](sarx_track_params& q) { q.confirm_hits = 6; }},
        {"window 33", [](sarx_track_params& q) { q.confirm_window = 33; }},
        {"window 0", [](sarx_track_params& q) { q.confirm_window = 0; q.confirm_hits = 0; }},
        {"misses negative", [](sarx_track_params& q) { q.max_misses = -1; }},
        {"tracks 0", [](sarx_track_params& q) { q.max_tracks = 0; }},
        {"tracks too many", [](sarx_track_params& q) { q.max_tracks = SARX_TRACK_MAX_TRACKS + 1; }},
        {"detections 0", [](sarx_track_params& q) { q.max_detections = 0; }},
        {"detections too many", [](sarx_track_params& q) { q.max_detections = SARX_TRACK_MAX_DETECTIONS + 1; }},
        {"reserved", [](sarx_track_params& q) { q.reserved = 1; }},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        size_t n = 12345;
        int rc = sarx_track_check(&p);
        if (rc != SARX_ERR_INVALID) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
        rc = sarx_track_table_bytes(&p, &n);
        if (rc != SARX_ERR_INVALID || n != 12345) { ++failures; fprintf(stderr, "FAIL table_bytes %s: rc %d\n", b.what, rc); }
        rc = sarx_track_workspace_bytes(&p, &n);
        if (rc != SARX_ERR_INVALID || n != 12345) { ++failures; fprintf(stderr, "FAIL workspace_bytes %s: rc %d\n", b.what, rc); }
    }
}

static void sizes() {
    sarx_track_params p = good();
    size_t n = 0;
    CHECK(sarx_track_table_bytes(&p, &n) == SARX_OK && n == 64 + (size_t)96 * 1024);
    CHECK(sarx_track_workspace_bytes(&p, &n) == SARX_OK && n == (size_t)4 * (2 * 1024 + 4096));
    p.max_tracks = 5; p.max_detections = 7;
    CHECK(sarx_track_table_bytes(&p, &n) == SARX_OK && n == 64 + 96 * 5);
    CHECK(sarx_track_workspace_bytes(&p, &n) == SARX_OK && n == (size_t)4 * (2 * 8 + 8));
    CHECK(sarx_track_table_bytes(&p, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_track_workspace_bytes(&p, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_track_table_bytes(nullptr, &n) == SARX_ERR_INVALID);
    CHECK(sarx_track_workspace_bytes(nullptr, &n) == SARX_ERR_INVALID);
}

static void launch_without_a_context() {
    sarx_track_params p = good();
    alignas(16) static char buf[4096];
    int32_t* assoc = (int32_t*)(buf + 2048);
    CHECK(sarx_track_init_dev(nullptr, &p, buf) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_track_init_dev(nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_track_init_dev(nullptr, &p, buf + 4) != SARX_OK);
    CHECK(sarx_track_step_dev(nullptr, &p, buf, 0, buf + 1024, assoc, buf + 3072) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_track_step_dev(nullptr, nullptr, nullptr, -1, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_track_step_dev(nullptr, &p, buf + 4, 0, buf + 1024, (int32_t*)(buf + 2049), buf + 3072) != SARX_OK);
    CHECK(sarx_track_step_dev(nullptr, &p, buf, -1, buf + 1024, nullptr, buf + 3072) != SARX_OK);
    CHECK(sarx_track_run_dev(nullptr, &p, buf, 16 + 48 * 4096, 2, buf + 1024, assoc, buf + 3072) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_track_run_dev(nullptr, nullptr, nullptr, 0, -1, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_track_run_dev(nullptr, &p, buf, 16, 2, buf + 1024, nullptr, buf + 3072) != SARX_OK);           // stride shorter than a slot
    CHECK(sarx_track_run_dev(nullptr, &p, buf, 16 + 48 * 4096 + 4, 2, buf + 1024, nullptr, buf + 3072) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    sizes();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "track_asan_test: %d failures\n", failures); return 1; }
    printf("track_asan_test: all checks passed\n");
    return 0;
}
