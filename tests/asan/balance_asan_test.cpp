// Host-side sanitizer test of the two-channel balance entry points (include/sarx_balance.h; `make asan-balance` in csrc/,
// tests/test_balance.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check and the two size
// queries, which need no device, are called with valid parameters and with every kind of bad one (block sizes, block count, mode,
// interp, min_count, reserved, clip, coherence, image size, NULL), and the two launch entry points with the arguments a careless
// caller would pass (NULL context, NULL parameters or buffers, misaligned buffers).  Every call must return an error code with a
// message - never crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_balance.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_balance_params good() {
    sarx_balance_params p{};
    p.block_az = 256; p.block_rg = 256; p.mode = SARX_BALANCE_LS; p.interp = SARX_BALANCE_BILINEAR;
    p.min_count = 16384; p.reserved = 0; p.clip_power = INFINITY; p.min_coherence = 0.0;
    return p;
}

static void parameter_check() {
    CHECK(sizeof(sarx_balance_params) == 40 && sizeof(sarx_balance_header) == 64 && sizeof(sarx_balance_record) == 64);
    sarx_balance_params p = good();
    CHECK(sarx_balance_check(&p, 8192, 8192) == SARX_OK);
    p.block_az = SARX_BALANCE_MIN_BLOCK; p.block_rg = SARX_BALANCE_MAX_BLOCK; p.mode = SARX_BALANCE_PHASE; p.interp = SARX_BALANCE_NEAREST;
    p.min_count = 1; p.clip_power = 1e-30; p.min_coherence = 1.0;
    CHECK(sarx_balance_check(&p, 8 * 65536, 4096) == SARX_OK);               // the limits themselves are allowed
    p = good();
    p.block_az = p.block_rg = 4096;
    CHECK(sarx_balance_check(&p, 1, 1) == SARX_OK);                          // a block larger than the image: one block
    CHECK(sarx_balance_check(nullptr, 1024, 1024) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* what; void (*edit)(sarx_balance_params&); int n_az, n_rg, code; } bad[] = {
        {"block_az 7", [](sarx_balance_params& q) { q.block_az = 7; }, 1024, 64, SARX_ERR_INVALID},
        {"block_rg 4097", [](sarx_balance_params& q) { q.block_rg = 4097; }, 1024, 64, SARX_ERR_INVALID},
        {"block_az 0", [](sarx_balance_params& q) { q.block_az = 0; }, 1024, 64, SARX_ERR_INVALID},
        {"block_rg negative", [](sarx_balance_params& q) { q.block_rg = -256; }, 1024, 64, SARX_ERR_INVALID},
        {"too many blocks", [](sarx_balance_params& q) { q.block_az = q.block_rg = 8; }, 2056, 2048, SARX_ERR_UNSUPPORTED},
        {"mode", [](sarx_balance_params& q) { q.mode = 2; }, 1024, 64, SARX_ERR_INVALID},
        {"interp", [](sarx_balance_params& q) { q.interp = -1; }, 1024, 64, SARX_ERR_INVALID},
        {"min_count 0", [](sarx_balance_params& q) { q.min_count = 0; }, 1024, 64, SARX_ERR_INVALID},
        {"reserved", [](sarx_balance_params& q) { q.reserved = 1; }, 1024, 64, SARX_ERR_INVALID},
        {"clip 0", [](sarx_balance_params& q) { q.clip_power = 0.0; }, 1024, 64, SARX_ERR_INVALID},
        {"clip NaN", [](sarx_balance_params& q) { q.clip_power = std::nan(""); }, 1024, 64, SARX_ERR_INVALID},
        {"clip negative", [](sarx_balance_params& q) { q.clip_power = -INFINITY; }, 1024, 64, SARX_ERR_INVALID},
        {"coherence 1.5", [](sarx_balance_params& q) { q.min_coherence = 1.5; }, 1024, 64, SARX_ERR_INVALID},
        {"coherence NaN", [](sarx_balance_params& q) { q.min_coherence = std::nan(""); }, 1024, 64, SARX_ERR_INVALID},
        {"image 0 rows", [](sarx_balance_params&) {}, 0, 64, SARX_ERR_INVALID},
        {"image -1 cols", [](sarx_balance_params&) {}, 1024, -1, SARX_ERR_INVALID},
        {"image too tall", [](sarx_balance_params& q) { q.block_az = 4096; }, (1 << 20) + 1, 64, SARX_ERR_UNSUPPORTED},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        size_t n = 12345;
        int rc = sarx_balance_check(&p, b.n_az, b.n_rg);
        if (rc != b.code) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
        rc = sarx_balance_table_bytes(&p, b.n_az, b.n_rg, &n);
        if (rc != b.code || n != 12345) { ++failures; fprintf(stderr, "FAIL table_bytes %s: rc %d\n", b.what, rc); }
        rc = sarx_balance_workspace_bytes(&p, b.n_az, b.n_rg, &n);
        if (rc != b.code || n != 12345) { ++failures; fprintf(stderr, "FAIL workspace_bytes %s: rc %d\n", b.what, rc); }
    }
}

static void sizes() {
    sarx_balance_params p = good();
    size_t n = 0;
    CHECK(sarx_balance_table_bytes(&p, 1000, 777, &n) == SARX_OK && n == 64 + 64 * 4 * 4);
    CHECK(sarx_balance_workspace_bytes(&p, 1000, 777, &n) == SARX_OK && n == (size_t)4 * 4 * 8 * 40);      // 8 strips of 32 rows per block
    p.block_az = 40; p.block_rg = 8;
    CHECK(sarx_balance_table_bytes(&p, 64, 64, &n) == SARX_OK && n == 64 + 64 * 2 * 8);
    CHECK(sarx_balance_workspace_bytes(&p, 64, 64, &n) == SARX_OK && n == (size_t)2 * 8 * 2 * 40);
    CHECK(sarx_balance_table_bytes(&p, 64, 64, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_balance_workspace_bytes(&p, 64, 64, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_balance_table_bytes(nullptr, 64, 64, &n) == SARX_ERR_INVALID);
    CHECK(sarx_balance_workspace_bytes(nullptr, 64, 64, &n) == SARX_ERR_INVALID);
}

static void launch_without_a_context() {
    sarx_balance_params p = good();
    alignas(16) static char buf[4096];
    float* plane = (float*)(buf + 2048);
    CHECK(sarx_balance_estimate_dev(nullptr, buf, buf, 1024, 64, &p, buf + 1024, buf + 2048) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_balance_estimate_dev(nullptr, nullptr, nullptr, 0, -1, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_balance_estimate_dev(nullptr, buf + 4, buf, 1024, 64, &p, buf + 1024, buf + 2048) != SARX_OK);
    CHECK(sarx_balance_apply_dev(nullptr, buf, buf, 1024, 64, &p, buf + 1024, buf, plane) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_balance_apply_dev(nullptr, nullptr, nullptr, 0, -1, nullptr, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_balance_apply_dev(nullptr, nullptr, buf, 1024, 64, &p, buf + 1024, buf, plane) != SARX_OK);     // dpca_mag without slc1
    CHECK(sarx_balance_apply_dev(nullptr, buf, buf, 1024, 64, &p, buf + 1024, buf + 3, nullptr) != SARX_OK);
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    sizes();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "balance_asan_test: %d failures\n", failures); return 1; }
    printf("balance_asan_test: all checks passed\n");
    return 0;
}
