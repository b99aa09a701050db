// Host-side sanitizer test of the N-receiver back-projection's and the multi-baseline resolver's entry points
// (include/sarx_tdbp_multi.h; `make asan-tdbpmulti` in csrc/, tests/test_tdbp_multi.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU, so no plan and no context can exist:
// every entry point is called with the arguments a careless caller would pass - each pointer NULL in turn, each channel pointer
// NULL in turn, both outputs NULL, misaligned outputs, NaN and infinite offsets, chirp centre and focus velocity, a bad scene size,
// a bad channel count, non-zero unused slots, bad pulse ranges, a NULL plan and a "plan" that sarx_tdbp_plan_create never returned
// (8 bytes of stack the sanitizer would catch a read past); the resolver's parameter block field by field, and its device entry
// point without a context.  The array of channel pointers holds exactly n_rx entries, so a read of an unused slot is caught.
// Every call must return SARX_ERR_INVALID with its message, never crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../include/sarx_tdbp_multi.h"

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

typedef int (*entry_fn)(sarx_tdbp_plan*, const void* const*, const double*, const double*, const double*, double, const double*, double,
                        const sarx_tdbp_multi_params*, void*, void*);

int main() {
    CHECK(sizeof(sarx_tdbp_multi_params) == 64);
    CHECK(sizeof(sarx_tdbp_multi_resolve_params) == 56);
    CHECK(sizeof(sarx_tdbp_multi_record) == 64);
    alignas(16) static char raw0[256], img128[4096], img64[4096];
    double pos[24] = {}, vel[24] = {}, tp[8] = {0, 1, 2, 3, 4, 5, 6, 7}, vf[3] = {0, 0, 0};
    for (int i = 0; i < 8; ++i) { pos[3 * i + 2] = 1.0; vel[3 * i] = 1.0; }
    const sarx_tdbp_multi_params good = {{-1.5, 1.5, 13.5, 0.0}, 1e-6, {5, 4, 0, 0}, 3, 3};
    const void* raws[3] = {raw0, raw0, raw0};                          // n_rx entries and no more
    alignas(8) char stale_bytes[8] = {};
    sarx_tdbp_plan* stale = (sarx_tdbp_plan*)stale_bytes;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    // the parameter block alone
    CHECK(sarx_tdbp_multi_check(8, &good) == SARX_OK);
    REFUSED(sarx_tdbp_multi_check(8, nullptr), "NULL");
    REFUSED(sarx_tdbp_multi_check(0, &good), "n_pulses");
    REFUSED(sarx_tdbp_multi_check(7, &good), "outside");               // pulses 5 .. 8 of seven
    for (int n : {1, 5, 0, -1, INT32_MAX, INT32_MIN}) { sarx_tdbp_multi_params k = good; k.n_rx = n; REFUSED(sarx_tdbp_multi_check(8, &k), "n_rx"); }
    { sarx_tdbp_multi_params k = good; k.rx_offset_m[3] = 1.0; REFUSED(sarx_tdbp_multi_check(8, &k), "unused"); }
    { sarx_tdbp_multi_params k = good; k.rx_offset_m[3] = nan; REFUSED(sarx_tdbp_multi_check(8, &k), "unused"); }
    { sarx_tdbp_multi_params k = good; k.first_pulse[3] = 1; REFUSED(sarx_tdbp_multi_check(8, &k), "unused"); }
    { sarx_tdbp_multi_params k = good; k.n_rx = 2; REFUSED(sarx_tdbp_multi_check(8, &k), "unused"); }
    for (double bad : {nan, inf, -inf}) {
        for (int ch = 0; ch < 3; ++ch) { sarx_tdbp_multi_params k = good; k.rx_offset_m[ch] = bad; REFUSED(sarx_tdbp_multi_check(8, &k), "rx_offset_m"); }
        sarx_tdbp_multi_params k = good; k.chirp_centre_s = bad; REFUSED(sarx_tdbp_multi_check(8, &k), "chirp_centre_s");
    }
    for (int n : {0, -1, INT32_MIN}) { sarx_tdbp_multi_params k = good; k.n_used = n; REFUSED(sarx_tdbp_multi_check(8, &k), "n_used"); }
    { sarx_tdbp_multi_params k = good; k.n_used = INT32_MAX; REFUSED(sarx_tdbp_multi_check(8, &k), "outside"); }
    { sarx_tdbp_multi_params k = good; k.first_pulse[1] = INT32_MAX; REFUSED(sarx_tdbp_multi_check(8, &k), "outside"); }
    for (int ch = 0; ch < 3; ++ch) { sarx_tdbp_multi_params k = good; k.first_pulse[ch] = -1; REFUSED(sarx_tdbp_multi_check(8, &k), "first_pulse"); }

    const entry_fn entries[2] = {sarx_tdbp_multi_dev, sarx_tdbp_multi_host};
    for (sarx_tdbp_plan* plan : {(sarx_tdbp_plan*)nullptr, stale})
        for (entry_fn f : entries) {
            // NULL pointers, one at a time (either output alone may be NULL)
            REFUSED(f(plan, nullptr, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raws, nullptr, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raws, pos, nullptr, tp, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raws, pos, vel, nullptr, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, nullptr, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, nullptr, img128, img64), "NULL");
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, nullptr, nullptr), "both outputs");
            for (int ch = 0; ch < 3; ++ch) {
                const void* one[3] = {raw0, raw0, raw0};
                one[ch] = nullptr;
                REFUSED(f(plan, one, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "channel");
            }
            // misaligned outputs
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, img128 + 8, img64), "misaligned");
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64 + 4), "misaligned");
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, nullptr, img64 + 1), "misaligned");
            // non-finite focus velocity, offsets and chirp centre
            for (double bad : {nan, inf, -inf}) {
                for (int i = 0; i < 3; ++i) {
                    vf[i] = bad;
                    REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, img128, nullptr), "vel_focus");
                    vf[i] = 0.0;
                }
                sarx_tdbp_multi_params k = good;
                k.rx_offset_m[2] = bad; REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &k, nullptr, img64), "rx_offset_m");
                k = good; k.chirp_centre_s = bad; REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &k, nullptr, img64), "chirp_centre_s");
            }
            for (double bad : {0.0, -1.0, nan, inf}) REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, bad, &good, img128, img64), "scene_size");
            // the channel count and the unused slots: refused before a channel pointer is read
            for (int n : {1, 5, INT32_MAX}) { sarx_tdbp_multi_params k = good; k.n_rx = n; REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &k, img128, img64), "n_rx"); }
            { sarx_tdbp_multi_params k = good; k.rx_offset_m[3] = 2.0; REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &k, img128, img64), "unused"); }
            // pulse ranges, as far as they can be judged without the plan's pulse count
            { sarx_tdbp_multi_params k = good; k.n_used = 0; REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &k, img128, img64), "n_used"); }
            { sarx_tdbp_multi_params k = good; k.first_pulse[1] = -3; REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &k, img128, img64), "first_pulse"); }
            // everything else in order: the plan itself
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "plan");
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, nullptr, img64), "plan");
            REFUSED(f(plan, raws, pos, vel, tp, 0.0, vf, 10.0, &good, img128, nullptr), "plan");
        }
    for (sarx_tdbp_plan* plan : {(sarx_tdbp_plan*)nullptr, stale}) {
        int tile = 7;
        REFUSED(sarx_tdbp_multi_route(plan, nullptr), "NULL");
        REFUSED(sarx_tdbp_multi_route(plan, &tile), "plan");
        CHECK(tile == 7);
        uint64_t bytes = 7, id = 7;
        REFUSED(sarx_tdbp_multi_scratch(plan, nullptr, &id), "NULL");
        REFUSED(sarx_tdbp_multi_scratch(plan, &bytes, nullptr), "NULL");
        REFUSED(sarx_tdbp_multi_scratch(plan, &bytes, &id), "plan");
        CHECK(bytes == 7 && id == 7);
    }
    CHECK(strstr(sarx_last_error(nullptr), "live") != nullptr);        // the last refusal was the stale plan's

    // the resolver's parameter block
    const sarx_tdbp_multi_resolve_params rgood = {{2e-4, 1e-3, 0.0}, 0.03, 30.0, 3, 1, 16, 0};
    CHECK(sarx_tdbp_multi_resolve_check(&rgood) == SARX_OK);
    REFUSED(sarx_tdbp_multi_resolve_check(nullptr), "NULL");
    for (int n : {1, 5, INT32_MIN}) { sarx_tdbp_multi_resolve_params k = rgood; k.n_rx = n; REFUSED(sarx_tdbp_multi_resolve_check(&k), "n_rx"); }
    for (double bad : {0.0, nan, inf, -inf})
        for (int b = 0; b < 2; ++b) { sarx_tdbp_multi_resolve_params k = rgood; k.lag_s[b] = bad; REFUSED(sarx_tdbp_multi_resolve_check(&k), "lag_s"); }
    { sarx_tdbp_multi_resolve_params k = rgood; k.lag_s[2] = 1e-3; REFUSED(sarx_tdbp_multi_resolve_check(&k), "unused"); }
    { sarx_tdbp_multi_resolve_params k = rgood; k.lag_s[2] = nan; REFUSED(sarx_tdbp_multi_resolve_check(&k), "unused"); }
    for (double bad : {0.0, -1.0, nan, inf}) {
        sarx_tdbp_multi_resolve_params k = rgood; k.wavelength_m = bad; REFUSED(sarx_tdbp_multi_resolve_check(&k), "wavelength_m");
        k = rgood; k.v_max_mps = bad; REFUSED(sarx_tdbp_multi_resolve_check(&k), "v_max_mps");
    }
    for (int h : {-1, 5, INT32_MAX}) { sarx_tdbp_multi_resolve_params k = rgood; k.half = h; REFUSED(sarx_tdbp_multi_resolve_check(&k), "half"); }
    for (int md : {0, -1, SARX_TDBP_MULTI_MAX_DETECTIONS + 1, INT32_MAX}) {
        sarx_tdbp_multi_resolve_params k = rgood; k.max_detections = md; REFUSED(sarx_tdbp_multi_resolve_check(&k), "max_detections");
    }
    { sarx_tdbp_multi_resolve_params k = rgood; k.reserved = 1; REFUSED(sarx_tdbp_multi_resolve_check(&k), "reserved"); }
    { sarx_tdbp_multi_resolve_params k = rgood; k.v_max_mps = 129.1 * 0.03 / 4e-3; REFUSED(sarx_tdbp_multi_resolve_check(&k), "candidates"); }
    { sarx_tdbp_multi_resolve_params k = rgood; k.v_max_mps = 1e300; REFUSED(sarx_tdbp_multi_resolve_check(&k), "candidates"); }
    { sarx_tdbp_multi_resolve_params k = rgood; k.v_max_mps = 128.9 * 0.03 / 4e-3; CHECK(sarx_tdbp_multi_resolve_check(&k) == SARX_OK); }
    REFUSED(sarx_tdbp_multi_resolve_dev(nullptr, &rgood, img64, 4, 4, img64, img128), "ctx");
    REFUSED(sarx_tdbp_multi_resolve_dev(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr), "ctx");

    sarx_ctx* ctx = nullptr;
    if (sarx_init(0, &ctx) == SARX_OK) {
        sarx_destroy(ctx);                                             // a box with a device: nothing more to check here
    } else {
        CHECK(ctx == nullptr);
        CHECK(strlen(sarx_last_error(nullptr)) > 5);
    }
    CHECK(sarx_tdbp_plan_destroy(nullptr) == SARX_OK);
    if (failures) { fprintf(stderr, "tdbpmulti_asan_test: %d failures\n", failures); return 1; }
    printf("tdbpmulti_asan_test: all checks passed\n");
    return 0;
}
