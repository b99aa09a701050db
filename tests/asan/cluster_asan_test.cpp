// Host-side sanitizer test of the GMTI plot extraction's entry points (include/sarx_cluster.h; `make asan-cluster` in csrc/,
// tests/test_cluster.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU: the parameter check and the size query,
// which need no device, are called with valid parameters and with every kind of bad one (links, members, capacities 0 and 16385,
// NULL), and the two launch entry points with the arguments a careless caller would pass (NULL context, NULL parameters or
// buffers, misaligned buffers, overlapping slots, strides shorter than a slot or no multiple of 8).  Every call must return an
// error code with a message - never crash.  Exit code 0 and no sanitizer report = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sarx_cluster.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static sarx_cluster_params good() {
    sarx_cluster_params p{};
    p.link_az = 4; p.link_rg = 6; p.min_members = 1; p.max_detections = 8;
    return p;
}

static void parameter_check() {
    CHECK(sizeof(sarx_cluster_params) == 16 && sizeof(sarx_cluster_plot) == 64);
    sarx_cluster_params p = good();
    CHECK(sarx_cluster_check(&p) == SARX_OK);
    p.link_az = p.link_rg = SARX_CLUSTER_MAX_LINK; p.max_detections = SARX_CLUSTER_MAX_DETECTIONS; p.min_members = 1 << 30;
    CHECK(sarx_cluster_check(&p) == SARX_OK);                                // the limits themselves are allowed
    p = good();
    p.link_az = p.link_rg = 0; p.max_detections = 1;
    CHECK(sarx_cluster_check(&p) == SARX_OK);
    CHECK(sarx_cluster_check(nullptr) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "NULL") != nullptr);
    struct { const char* what; void (*edit)(sarx_cluster_params&); } bad[] = {
        {"link_az negative", [](sarx_cluster_params& q) { q.link_az = -1; }},
        {"link_rg negative", [](sarx_cluster_params& q) { q.link_rg = -1; }},
        {"link_az 65", [](sarx_cluster_params& q) { q.link_az = SARX_CLUSTER_MAX_LINK + 1; }},
        {"link_rg 65", [](sarx_cluster_params& q) { q.link_rg = SARX_CLUSTER_MAX_LINK + 1; }},
        {"members 0", [](sarx_cluster_params& q) { q.min_members = 0; }},
        {"members negative", [](sarx_cluster_params& q) { q.min_members = -3; }},
        {"capacity 0", [](sarx_cluster_params& q) { q.max_detections = 0; }},
        {"capacity negative", [](sarx_cluster_params& q) { q.max_detections = -1; }},
        {"capacity 16385", [](sarx_cluster_params& q) { q.max_detections = SARX_CLUSTER_MAX_DETECTIONS + 1; }},
    };
    for (auto& b : bad) {
        p = good();
        b.edit(p);
        size_t n = 12345;
        int rc = sarx_cluster_check(&p);
        if (rc != SARX_ERR_INVALID) { ++failures; fprintf(stderr, "FAIL %s: rc %d\n", b.what, rc); }
        CHECK(strlen(sarx_last_error(nullptr)) > 10);
        rc = sarx_cluster_plots_bytes(&p, &n);
        if (rc != SARX_ERR_INVALID || n != 12345) { ++failures; fprintf(stderr, "FAIL plots_bytes %s: rc %d\n", b.what, rc); }
        alignas(16) static char buf[2048];
        CHECK(sarx_cluster_step_dev(nullptr, &p, buf, buf + 1024, nullptr, nullptr) != SARX_OK);
        CHECK(sarx_cluster_run_dev(nullptr, &p, buf, 512, buf + 1024, 512, 1, nullptr, 0, nullptr) != SARX_OK);
    }
}

static void sizes() {
    sarx_cluster_params p = good();
    size_t n = 0;
    CHECK(sarx_cluster_plots_bytes(&p, &n) == SARX_OK && n == 64 * 8);
    p.max_detections = SARX_CLUSTER_MAX_DETECTIONS;
    CHECK(sarx_cluster_plots_bytes(&p, &n) == SARX_OK && n == (size_t)64 * 16384);
    CHECK(sarx_cluster_plots_bytes(&p, nullptr) == SARX_ERR_INVALID);
    CHECK(sarx_cluster_plots_bytes(nullptr, &n) == SARX_ERR_INVALID);
}

static void launch_without_a_context() {
    sarx_cluster_params p = good();                  // slot: 16 + 48 * 8 = 400 bytes, plot records 512, labels 32
    alignas(16) static char buf[8192];
    char* in = buf; char* out = buf + 1024; char* plots = buf + 2048; int32_t* labels = (int32_t*)(buf + 4096);
    CHECK(sarx_cluster_step_dev(nullptr, &p, in, out, plots, labels) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_cluster_step_dev(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_cluster_step_dev(nullptr, &p, nullptr, out, plots, labels) != SARX_OK);
    CHECK(sarx_cluster_step_dev(nullptr, &p, in, nullptr, nullptr, nullptr) != SARX_OK);
    CHECK(sarx_cluster_step_dev(nullptr, &p, in + 4, out, plots, labels) != SARX_OK);                    // misaligned
    CHECK(sarx_cluster_step_dev(nullptr, &p, in, out, plots + 4, (int32_t*)(buf + 4097)) != SARX_OK);
    CHECK(sarx_cluster_step_dev(nullptr, &p, in, in, plots, labels) != SARX_OK);                         // in place
    CHECK(sarx_cluster_step_dev(nullptr, &p, in, in + 392, plots, labels) != SARX_OK);                   // the last 8 bytes shared
    CHECK(sarx_cluster_step_dev(nullptr, &p, in, out, in + 8, labels) != SARX_OK);
    CHECK(sarx_cluster_step_dev(nullptr, &p, in, out, plots, (int32_t*)(out + 16)) != SARX_OK);
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 400, out, 400, 2, plots, 512, labels) == SARX_ERR_INVALID);
    CHECK(strstr(sarx_last_error(nullptr), "ctx") != nullptr);
    CHECK(sarx_cluster_run_dev(nullptr, nullptr, nullptr, 0, nullptr, 0, -1, nullptr, 0, nullptr) != SARX_OK);
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 16, out, 400, 2, nullptr, 0, nullptr) != SARX_OK);         // stride shorter than a slot
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 400, out, 392, 2, nullptr, 0, nullptr) != SARX_OK);
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 404, out, 400, 2, nullptr, 0, nullptr) != SARX_OK);        // no multiple of 8
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 400, out, 400, 2, plots, 504, nullptr) != SARX_OK);        // plot stride too short
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 400, out, 400, -1, nullptr, 0, nullptr) != SARX_OK);
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 400, in + 400, 400, 2, nullptr, 0, nullptr) != SARX_OK);   // the second input slot IS the first output slot
    CHECK(sarx_cluster_run_dev(nullptr, &p, in, 400, out, 400, 0, nullptr, 0, nullptr) != SARX_OK);        // NULL ctx even with nothing to do
    CHECK(strlen(sarx_last_error(nullptr)) > 5);
}

int main() {
    parameter_check();
    sizes();
    launch_without_a_context();
    if (failures) { fprintf(stderr, "cluster_asan_test: %d failures\n", failures); return 1; }
    printf("cluster_asan_test: all checks passed\n");
    return 0;
}
