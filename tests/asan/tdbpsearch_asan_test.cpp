// Host-side sanitizer test of the focus-velocity search's entry points (include/sarx_tdbp_search.h; `make asan-tdbpsearch` in
// csrc/, tests/test_tdbp_search.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU, so no plan can exist: every entry
// point is called with the arguments a careless caller would pass - each pointer NULL in turn, n_hyp 0, negative and 1025, NaN and
// infinite velocities, a bad scene size, a NULL plan, and a "plan" that sarx_tdbp_plan_create never returned (a destroyed one looks
// the same to the library: it is not in the list of live plans, and is refused without being read - the fake one here is 8 bytes
// of stack the sanitizer would catch a read past).  Every call must return SARX_ERR_INVALID with its message, never crash.
// Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/sarx_tdbp_search.h"

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define REFUSED(call, word)                                                         \
    do {                                                                            \
        CHECK((call) == SARX_ERR_INVALID);                                          \
        CHECK(strstr(sarx_last_error(nullptr), word) != nullptr);                   \
    } while (0)

int main() {
    CHECK(sizeof(sarx_tdbp_search_record) == 32);
    CHECK(SARX_TDBP_SEARCH_MAX_HYP == 1024);
    alignas(16) static char raw[256], img[4096];
    double pos[6] = {0, 0, 1, 0, 0, 1}, vel[6] = {1, 0, 0, 1, 0, 0}, tp[2] = {0, 1};
    std::vector<double> hyps(3 * (SARX_TDBP_SEARCH_MAX_HYP + 1), 1.0);
    std::vector<sarx_tdbp_search_record> rec(SARX_TDBP_SEARCH_MAX_HYP + 1);
    alignas(8) char stale_bytes[8] = {};
    sarx_tdbp_plan* stale = (sarx_tdbp_plan*)stale_bytes;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    for (sarx_tdbp_plan* plan : {(sarx_tdbp_plan*)nullptr, stale}) {
        // NULL pointers, one at a time (images may be NULL: it is optional)
        REFUSED(sarx_tdbp_search_dev(plan, nullptr, pos, vel, tp, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_dev(plan, raw, nullptr, vel, tp, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_dev(plan, raw, pos, nullptr, tp, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, nullptr, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, tp, 0.0, nullptr, 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, tp, 0.0, hyps.data(), 2, 10.0, img, nullptr), "NULL");
        REFUSED(sarx_tdbp_search_host(plan, nullptr, pos, vel, tp, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_host(plan, raw, nullptr, vel, tp, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_host(plan, raw, pos, nullptr, tp, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, nullptr, 0.0, hyps.data(), 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, tp, 0.0, nullptr, 2, 10.0, img, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, tp, 0.0, hyps.data(), 2, 10.0, nullptr, nullptr), "NULL");
        REFUSED(sarx_tdbp_search_metric_dev(plan, nullptr, 2, rec.data()), "NULL");
        REFUSED(sarx_tdbp_search_metric_dev(plan, img, 2, nullptr), "NULL");
        REFUSED(sarx_tdbp_search_route(plan, nullptr), "NULL");
        // n_hyp
        for (int n : {0, -1, INT32_MIN, SARX_TDBP_SEARCH_MAX_HYP + 1, INT32_MAX}) {
            REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, tp, 0.0, hyps.data(), n, 10.0, nullptr, rec.data()), "n_hyp");
            REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, tp, 0.0, hyps.data(), n, 10.0, nullptr, rec.data()), "n_hyp");
            REFUSED(sarx_tdbp_search_metric_dev(plan, img, n, rec.data()), "n_hyp");
        }
        // non-finite velocities: the first, the last, every component
        for (double bad : {nan, inf, -inf})
            for (size_t at : {(size_t)0, (size_t)1, (size_t)2, (size_t)3 * SARX_TDBP_SEARCH_MAX_HYP - 1}) {
                hyps[at] = bad;
                REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, tp, 0.0, hyps.data(), SARX_TDBP_SEARCH_MAX_HYP, 10.0, nullptr, rec.data()), "non-finite");
                REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, tp, 0.0, hyps.data(), SARX_TDBP_SEARCH_MAX_HYP, 10.0, nullptr, rec.data()), "non-finite");
                hyps[at] = 1.0;
            }
        // scene size
        for (double bad : {0.0, -1.0, nan, inf}) {
            REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, tp, 0.0, hyps.data(), 2, bad, nullptr, rec.data()), "scene_size");
            REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, tp, 0.0, hyps.data(), 2, bad, nullptr, rec.data()), "scene_size");
        }
        // chunks
        REFUSED(sarx_tdbp_search_set_chunks(plan, -1), "chunks");
        REFUSED(sarx_tdbp_search_set_chunks(plan, SARX_TDBP_SEARCH_MAX_CHUNKS + 1), "chunks");
        // everything else in order: the plan itself
        int tile = 7;
        REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, tp, 0.0, hyps.data(), SARX_TDBP_SEARCH_MAX_HYP, 10.0, img, rec.data()), "plan");
        REFUSED(sarx_tdbp_search_dev(plan, raw, pos, vel, tp, 0.0, hyps.data(), 1, 10.0, nullptr, rec.data()), "plan");
        REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, tp, 0.0, hyps.data(), 3, 10.0, img, rec.data()), "plan");
        REFUSED(sarx_tdbp_search_host(plan, raw, pos, vel, tp, 0.0, hyps.data(), 3, 10.0, nullptr, rec.data()), "plan");
        REFUSED(sarx_tdbp_search_metric_dev(plan, img, 1, rec.data()), "plan");
        REFUSED(sarx_tdbp_search_route(plan, &tile), "plan");
        REFUSED(sarx_tdbp_search_set_chunks(plan, 0), "plan");
        REFUSED(sarx_tdbp_search_set_chunks(plan, SARX_TDBP_SEARCH_MAX_CHUNKS), "plan");
        CHECK(tile == 7);
    }
    CHECK(strstr(sarx_last_error(nullptr), "live") != nullptr);        // the last refusal was the stale plan's
    // no device: no context, so no plan; destroying nothing is allowed
    sarx_ctx* ctx = nullptr;
    if (sarx_init(0, &ctx) == SARX_OK) {
        sarx_destroy(ctx);                                             // a box with a device: nothing more to check here
    } else {
        CHECK(ctx == nullptr);
        CHECK(strlen(sarx_last_error(nullptr)) > 5);
        sarx_tdbp_plan* plan = (sarx_tdbp_plan*)stale_bytes;
        sarx_tdbp_params k = {299792458.0, 9.65e9, 60e6, 2e-6, 25e12};
        CHECK(sarx_tdbp_plan_create(nullptr, 8, 128, 8, 8, &k, &plan) != SARX_OK);
    }
    CHECK(sarx_tdbp_plan_destroy(nullptr) == SARX_OK);
    if (failures) { fprintf(stderr, "tdbpsearch_asan_test: %d failures\n", failures); return 1; }
    printf("tdbpsearch_asan_test: all checks passed\n");
    return 0;
}
