// Host-side sanitizer test of the entry points of the focus-velocity search on the two-receiver back-projection
// (include/sarx_tdbp_pair_search.h; `make asan-tdbppairsearch` in csrc/, tests/test_tdbp_pair_search.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU, so no plan can exist: every entry
// point is called with the arguments a careless caller would pass - each pointer NULL in turn, misaligned slot and outputs, n_hyp and
// chip sizes out of range, an unknown source, no room for a report, too many chips, NaN and infinite focus velocities, a bad scene
// size, bad pair parameters, a NULL plan, and a "plan" that sarx_tdbp_plan_create never returned (8 bytes of stack the sanitizer
// would catch a read past).  Every call must return SARX_ERR_INVALID with its message, in the order the header gives, never
// crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../include/sarx_tdbp_pair_search.h"

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

typedef int (*entry_fn)(sarx_tdbp_plan*, const void*, const void*, const double*, const double*, const double*, double, double,
                        const sarx_tdbp_pair_params*, const double*, const sarx_gmti_report*, const sarx_gmti_header*, int,
                        const sarx_tdbp_pair_search_params*, sarx_tdbp_search_record*, sarx_tdbp_pair_search_best*, void*);

int main() {
    CHECK(sizeof(sarx_tdbp_pair_search_params) == 16);
    CHECK(sizeof(sarx_tdbp_pair_search_best) == 80);
    CHECK(sizeof(sarx_tdbp_search_record) == 32);
    alignas(16) static char raw0[256], raw1[256], slot[16 + 4 * 48], recs[4 * 3 * 32], bests[4 * 80], chips[4096];
    double pos[6] = {0, 0, 1, 0, 0, 1}, vel[6] = {1, 0, 0, 1, 0, 0}, tp[2] = {0, 1};
    double hyps[9] = {0, 0, 0, 1, 0, 0, 2, 0, 0};
    const sarx_tdbp_pair_params pair = {{-1.5, 1.5}, 1e-6, {1, 0}, 1, 0};
    const sarx_tdbp_pair_search_params good = {16, 24, 3, SARX_TDBP_PAIR_SEARCH_DPCA};
    const sarx_gmti_header* hdr = (const sarx_gmti_header*)slot;
    const sarx_gmti_report* rep = (const sarx_gmti_report*)(slot + 16);
    sarx_tdbp_search_record* rec = (sarx_tdbp_search_record*)recs;
    sarx_tdbp_pair_search_best* best = (sarx_tdbp_pair_search_best*)bests;
    alignas(8) char stale_bytes[8] = {};
    sarx_tdbp_plan* stale = (sarx_tdbp_plan*)stale_bytes;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    // the parameter block alone, and against a grid
    CHECK(sarx_tdbp_pair_search_check(&good, 0, 0) == SARX_OK);
    CHECK(sarx_tdbp_pair_search_check(&good, 16, 24) == SARX_OK);
    REFUSED(sarx_tdbp_pair_search_check(nullptr, 0, 0), "NULL");
    REFUSED(sarx_tdbp_pair_search_check(&good, -1, 0), "negative");
    REFUSED(sarx_tdbp_pair_search_check(&good, 15, 24), "larger than the grid");
    REFUSED(sarx_tdbp_pair_search_check(&good, 16, 23), "larger than the grid");
    for (int n : {0, -1, SARX_TDBP_PAIR_SEARCH_MAX_HYP + 1, INT32_MAX, INT32_MIN}) {
        sarx_tdbp_pair_search_params k = good; k.n_hyp = n; REFUSED(sarx_tdbp_pair_search_check(&k, 0, 0), "n_hyp");
    }
    for (int n : {3, 0, -16, SARX_TDBP_PAIR_SEARCH_MAX_CHIP + 1, INT32_MAX}) {
        sarx_tdbp_pair_search_params k = good; k.chip_x = n; REFUSED(sarx_tdbp_pair_search_check(&k, 0, 0), "chip");
        k = good; k.chip_y = n; REFUSED(sarx_tdbp_pair_search_check(&k, 0, 0), "chip");
    }
    for (int n : {-1, 2, INT32_MAX}) { sarx_tdbp_pair_search_params k = good; k.source = n; REFUSED(sarx_tdbp_pair_search_check(&k, 0, 0), "source"); }
    { sarx_tdbp_pair_search_params k = good; k.chip_x = 4; k.chip_y = 64; k.n_hyp = 64; k.source = SARX_TDBP_PAIR_SEARCH_CH0;
      CHECK(sarx_tdbp_pair_search_check(&k, 4, 64) == SARX_OK); }

    const entry_fn entries[2] = {sarx_tdbp_pair_search_dev, sarx_tdbp_pair_search_host};
    for (sarx_tdbp_plan* plan : {(sarx_tdbp_plan*)nullptr, stale})
        for (entry_fn f : entries) {
            // NULL pointers, one at a time (the chips alone may be NULL)
            REFUSED(f(plan, nullptr, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, nullptr, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, nullptr, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, nullptr, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, nullptr, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, nullptr, hyps, rep, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, nullptr, rep, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, nullptr, hdr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, nullptr, 4, &good, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, nullptr, rec, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, nullptr, best, chips), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, nullptr, chips), "NULL");
            // misaligned slot and outputs
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, (const sarx_gmti_report*)(slot + 20), hdr, 4, &good, rec, best, chips), "misaligned");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, (const sarx_gmti_header*)(slot + 2), 4, &good, rec, best, chips), "misaligned");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, (sarx_tdbp_search_record*)(recs + 4), best, chips), "misaligned");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, (sarx_tdbp_pair_search_best*)(bests + 4), chips), "misaligned");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, chips + 8), "misaligned");
            // the search's own parameters
            { sarx_tdbp_pair_search_params k = good; k.n_hyp = 0; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &k, rec, best, chips), "n_hyp"); }
            { sarx_tdbp_pair_search_params k = good; k.n_hyp = 65; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &k, rec, best, chips), "n_hyp"); }
            { sarx_tdbp_pair_search_params k = good; k.chip_x = 3; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &k, rec, best, chips), "chip"); }
            { sarx_tdbp_pair_search_params k = good; k.chip_y = 65; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &k, rec, best, chips), "chip"); }
            { sarx_tdbp_pair_search_params k = good; k.source = 2; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &k, rec, best, chips), "source"); }
            for (int md : {0, -1, INT32_MIN}) REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, md, &good, rec, best, chips), "max_detections");
            for (int md : {21846, INT32_MAX}) REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, md, &good, rec, best, chips), "chips, more than");
            // non-finite focus velocities
            for (double bad : {nan, inf, -inf})
                for (int i = 0; i < 9; ++i) {
                    const double was = hyps[i];
                    hyps[i] = bad;
                    REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, nullptr), "focus velocity");
                    hyps[i] = was;
                }
            // scene size
            for (double bad : {0.0, -1.0, nan, inf}) REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, bad, &pair, hyps, rep, hdr, 4, &good, rec, best, chips), "scene_size");
            // the pair's parameters, as far as they can be judged without the plan's pulse count
            for (double bad : {nan, inf}) {
                sarx_tdbp_pair_params k = pair;
                k.rx_offset_m[1] = bad; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &k, hyps, rep, hdr, 4, &good, rec, best, chips), "rx_offset_m");
                k = pair; k.chirp_centre_s = bad; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &k, hyps, rep, hdr, 4, &good, rec, best, chips), "chirp_centre_s");
            }
            { sarx_tdbp_pair_params k = pair; k.n_used = 0; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &k, hyps, rep, hdr, 4, &good, rec, best, chips), "n_used"); }
            { sarx_tdbp_pair_params k = pair; k.first_pulse[1] = -3; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &k, hyps, rep, hdr, 4, &good, rec, best, chips), "first_pulse"); }
            // everything else in order: the plan itself
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, chips), "plan");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, 10.0, &pair, hyps, rep, hdr, 4, &good, rec, best, nullptr), "plan");
        }
    for (sarx_tdbp_plan* plan : {(sarx_tdbp_plan*)nullptr, stale}) {
        int tile = 7;
        REFUSED(sarx_tdbp_pair_search_route(plan, nullptr), "NULL");
        REFUSED(sarx_tdbp_pair_search_route(plan, &tile), "plan");
        CHECK(tile == 7);
    }
    CHECK(strstr(sarx_last_error(nullptr), "live") != nullptr);        // the last refusal was the stale plan's
    sarx_ctx* ctx = nullptr;
    if (sarx_init(0, &ctx) == SARX_OK) {
        sarx_destroy(ctx);                                             // a box with a device: nothing more to check here
    } else {
        CHECK(ctx == nullptr);
        CHECK(strlen(sarx_last_error(nullptr)) > 5);
    }
    CHECK(sarx_tdbp_plan_destroy(nullptr) == SARX_OK);
    if (failures) { fprintf(stderr, "tdbppairsearch_asan_test: %d failures\n", failures); return 1; }
    printf("tdbppairsearch_asan_test: all checks passed\n");
    return 0;
}
