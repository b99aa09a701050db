// Host-side sanitizer test of the Kalman ground tracker's entry points (include/sarx_ktrack.h; `make asan-ktrack` in csrc/,
// tests/test_ktrack.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check and the two size
// queries, which need no device, are called with valid parameters and with every kind of bad one (sigmas, q, gates, birth ratio,
// confirmation rule, misses, capacities, reserved, NULL), and the three launch entry points with the arguments a careless caller
// would pass (NULL context, NULL parameters, frames or buffers, misaligned buffers, bad strides, a frame array shorter than
// n_frames is not among them: the array is the caller's).  Every call must return an error code with a message - never crash.
// Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_ktrack.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_ktrack_params good() {
    sarx_ktrack_params p{};
    p.sigma_pos = 1.0; p.sigma_v = 0.3; p.sigma_v_tan = 10.0; p.q = 0.01; p.gate_d2 = 16.27; p.gate_m = 100.0; p.birth_ratio = 0.0;
    p.confirm_hits = 3; p.confirm_window = 5; p.max_misses = 3; p.max_tracks = 1024; p.max_detections = 4096; p.reserved = 0;
    return p;
}

static sarx_ktrack_frame good_frame() {
    sarx_ktrack_frame f{};
    f.t = 2.0; f.pos_ref[0] = 5000.0; f.pos_ref[2] = 3000.0; f.vel_ref[1] = 218.0; f.frame_index = 1;
    return f;
}

static void parameter_check() {
    CHECK(sizeof(sarx_ktrack_params) == 80 && sizeof(sarx_ktrack_frame) == 64 && sizeof(sarx_ktrack_header) == 64 &&
          sizeof(sarx_ktrack_slot) == 192);
    sarx_ktrack_params p = good();
    CHECK(sarx_ktrack_check(&p) == SARX_OK);
    p.q = 0.0; p.birth_ratio = 1e300; p.sigma_pos = 1e-300; p.confirm_hits = 32; p.confirm_window = 32; p.max_misses = 0;
    p.max_tracks = SARX_KTRACK_MAX_TRACKS; p.max_detections = SARX_KTRACK_MAX_DETECTIONS;
    CHECK(sarx_ktrack_check(&p) == SARX_OK);                                 // the limits themselves are allowed
    p = good();
    p.confirm_hits = p.confirm_window = 1; p.max_tracks = 1; p.max_detections = 1;
    CHECK(sarx_ktrack_check(&p) == SARX_OK);
    CHECK(sarx_ktrack_check(nullptr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* word; void (*edit)(sarx_ktrack_params&); } bad[] = {
        {"sigma_pos", [](sarx_ktrack_params& q) { q.sigma_pos = 0.0; }},
        {"sigma_pos", [](sarx_ktrack_params& q) { q.sigma_pos = std::nan(""); }},
        {"sigma_v ", [](sarx_ktrack_params& q) { q.sigma_v = -0.3; }},
        {"sigma_v ", [](sarx_ktrack_params& q) { q.sigma_v = INFINITY; }},
        {"sigma_v_tan", [](sarx_ktrack_params& q) { q.sigma_v_tan = 0.0; }},
        {"sigma_v_tan", [](sarx_ktrack_params& q) { q.sigma_v_tan = std::nan(""); }},
        {"q ", [](sarx_ktrack_params& q) { q.q = -1e-300; }},
        {"q ", [](sarx_ktrack_params& q) { q.q = INFINITY; }},
        {"gate_d2", [](sarx_ktrack_params& q) { q.gate_d2 = 0.0; }},
        {"gate_d2", [](sarx_ktrack_params& q) { q.gate_d2 = std::nan(""); }},
        {"gate_m", [](sarx_ktrack_params& q) { q.gate_m = -1.0; }},
        {"gate_m", [](sarx_ktrack_params& q) { q.gate_m = INFINITY; }},
        {"birth_ratio", [](sarx_ktrack_params& q) { q.birth_ratio = -1.0; }},
        {"birth_ratio", [](sarx_ktrack_params& q) { q.birth_ratio = INFINITY; }},
        {"confirm_hits", [](sarx_ktrack_params& q) { q.confirm_hits = 0; }},
        {"confirm_hits", [](sarx_ktrack_params& q) { q.confirm_hits = 6; }},
        {"confirm_window", [](sarx_ktrack_params& q) { q.confirm_window = 33; }},
        {"confirm_window", [](sarx_ktrack_params& q) { q.confirm_window = 0; q.confirm_hits = 0; }},
        {"max_misses", [](sarx_ktrack_params& q) { q.max_misses = -1; }},
        {"max_tracks", [](sarx_ktrack_params& q) { q.max_tracks = 0; }},
        {"max_tracks", [](sarx_ktrack_params& q) { q.max_tracks = SARX_KTRACK_MAX_TRACKS + 1; }},
        {"max_detections", [](sarx_ktrack_params& q) { q.max_detections = 0; }},
        {"max_detections", [](sarx_ktrack_params& q) { q.max_detections = SARX_KTRACK_MAX_DETECTIONS + 1; }},
        {"reserved", [](sarx_ktrack_params& q) { q.reserved = 1; }},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        size_t n = 12345;
        int rc = sarx_ktrack_check(&p);
        if (rc != SARX_ERR_INVALID || !strstr(sarx_last_error(nullptr), b.word)) {
            ++failures;
            fprintf(stderr, "FAIL %s: rc %d, \"%s\"\n", b.word, rc, sarx_last_error(nullptr));
        }
        rc = sarx_ktrack_table_bytes(&p, &n);
        if (rc != SARX_ERR_INVALID || n != 12345) { ++failures; fprintf(stderr, "FAIL table_bytes %s: rc %d\n", b.word, rc); }
        rc = sarx_ktrack_workspace_bytes(&p, &n);
        if (rc != SARX_ERR_INVALID || n != 12345) { ++failures; fprintf(stderr, "FAIL workspace_bytes %s: rc %d\n", b.word, rc); }
    }
}

static void sizes() {
    sarx_ktrack_params p = good();
    size_t n = 0;
    CHECK(sarx_ktrack_table_bytes(&p, &n) == SARX_OK && n == 64 + (size_t)192 * 1024);
    CHECK(sarx_ktrack_workspace_bytes(&p, &n) == SARX_OK && n == (size_t)8 * (15 * 1024 + 11 * 4096) + (size_t)4 * (2 * 1024 + 4096));
    p.max_tracks = 257; p.max_detections = 7;                                // capacities are padded to whole stages of 256
    CHECK(sarx_ktrack_table_bytes(&p, &n) == SARX_OK && n == 64 + 192 * 257);
    CHECK(sarx_ktrack_workspace_bytes(&p, &n) == SARX_OK && n == (size_t)8 * (15 * 512 + 11 * 256) + (size_t)4 * (2 * 512 + 256));
    CHECK(sarx_ktrack_table_bytes(&p, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_ktrack_workspace_bytes(&p, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_ktrack_table_bytes(nullptr, &n) == SARX_ERR_INVALID);
    CHECK(sarx_ktrack_workspace_bytes(nullptr, &n) == SARX_ERR_INVALID);
}

static void launch_without_a_context() {
    sarx_ktrack_params p = good();
    sarx_ktrack_frame f = good_frame();
    sarx_ktrack_frame two[2] = {good_frame(), good_frame()};
    alignas(16) static char buf[8192];
    int32_t* assoc = (int32_t*)(buf + 2048);
    CHECK(sarx_ktrack_init_dev(nullptr, &p, buf) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_ktrack_init_dev(nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_ktrack_init_dev(nullptr, &p, buf + 4) != SARX_OK);
    CHECK(sarx_ktrack_step_dev(nullptr, &p, &f, buf, buf + 512, buf + 1024, 8, buf + 4096, assoc, buf + 6144) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_ktrack_step_dev(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_ktrack_step_dev(nullptr, &p, nullptr, buf, buf + 512, buf + 1024, 8, buf + 4096, assoc, buf + 6144) != SARX_OK);
    CHECK(sarx_ktrack_step_dev(nullptr, &p, &f, buf + 4, buf + 512, buf + 1028, 12, buf + 4096, (int32_t*)(buf + 2049), buf + 6144) != SARX_OK);
    f.t = std::nan("");
    CHECK(sarx_ktrack_step_dev(nullptr, &p, &f, buf, buf + 512, buf + 1024, 8, buf + 4096, nullptr, buf + 6144) != SARX_OK);
    f = good_frame();
    f.frame_index = -1;
    CHECK(sarx_ktrack_step_dev(nullptr, &p, &f, buf, buf + 512, buf + 1024, 8, buf + 4096, nullptr, buf + 6144) != SARX_OK);
    const size_t slot = 16 + (size_t)48 * 4096, recs = (size_t)64 * 4096, speeds = (size_t)8 * 4096;
    CHECK(sarx_ktrack_run_dev(nullptr, &p, two, 2, buf, slot, buf + 512, recs, buf + 1024, 8, speeds, buf + 4096, assoc, buf + 6144) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_ktrack_run_dev(nullptr, nullptr, nullptr, -1, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_ktrack_run_dev(nullptr, &p, nullptr, 2, buf, slot, buf + 512, recs, buf + 1024, 8, speeds, buf + 4096, nullptr, buf + 6144) != SARX_OK);
    CHECK(sarx_ktrack_run_dev(nullptr, &p, two, 2, buf, 16, buf + 512, recs, buf + 1024, 8, speeds, buf + 4096, nullptr, buf + 6144) != SARX_OK);
    CHECK(sarx_ktrack_run_dev(nullptr, &p, two, 2, buf, slot, buf + 512, recs - 64, buf + 1024, 8, speeds, buf + 4096, nullptr, buf + 6144) != SARX_OK);
    CHECK(sarx_ktrack_run_dev(nullptr, &p, two, 2, buf, slot, buf + 512, recs, buf + 1024, 64, speeds, buf + 4096, nullptr, buf + 6144) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    sizes();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "ktrack_asan_test: %d failures\n", failures); return 1; }
    printf("ktrack_asan_test: all checks passed\n");
    return 0;
}
