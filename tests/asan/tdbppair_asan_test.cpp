// Host-side sanitizer test of the two-receiver back-projection's entry points (include/sarx_tdbp_pair.h; `make asan-tdbppair` in
// csrc/, tests/test_tdbp_pair.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU, so no plan can exist: every entry
// point is called with the arguments a careless caller would pass - each pointer NULL in turn, both outputs NULL, misaligned
// outputs, NaN and infinite offsets, chirp centre and focus velocity, a bad scene size, bad pulse ranges, a NULL plan, and a "plan"
// that sarx_tdbp_plan_create never returned (a destroyed one looks the same to the library: it is not in the list of live plans,
// and is refused without being read - the fake one here is 8 bytes of stack the sanitizer would catch a read past).  Every call
// must return SARX_ERR_INVALID with its message, never crash.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../include/sarx_tdbp_pair.h"

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

typedef int (*entry_fn)(sarx_tdbp_plan*, const void*, const void*, const double*, const double*, const double*, double, const double*,
                        double, const sarx_tdbp_pair_params*, void*, void*);

int main() {
    CHECK(sizeof(sarx_tdbp_pair_params) == 40);
    alignas(16) static char raw0[256], raw1[256], img128[4096], img64[4096];
    double pos[6] = {0, 0, 1, 0, 0, 1}, vel[6] = {1, 0, 0, 1, 0, 0}, tp[2] = {0, 1}, vf[3] = {0, 0, 0};
    const sarx_tdbp_pair_params good = {{-1.5, 1.5}, 1e-6, {1, 0}, 1, 0};
    alignas(8) char stale_bytes[8] = {};
    sarx_tdbp_plan* stale = (sarx_tdbp_plan*)stale_bytes;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    // the parameter block alone
    CHECK(sarx_tdbp_pair_check(2, &good) == SARX_OK);
    REFUSED(sarx_tdbp_pair_check(2, nullptr), "NULL");
    REFUSED(sarx_tdbp_pair_check(0, &good), "n_pulses");
    REFUSED(sarx_tdbp_pair_check(1, &good), "outside");                  // pulses 1 .. 2 of one
    for (double bad : {nan, inf, -inf}) {
        sarx_tdbp_pair_params k = good;
        k.rx_offset_m[0] = bad; REFUSED(sarx_tdbp_pair_check(2, &k), "rx_offset_m");
        k = good; k.rx_offset_m[1] = bad; REFUSED(sarx_tdbp_pair_check(2, &k), "rx_offset_m");
        k = good; k.chirp_centre_s = bad; REFUSED(sarx_tdbp_pair_check(2, &k), "chirp_centre_s");
    }
    for (int n : {0, -1, INT32_MIN}) { sarx_tdbp_pair_params k = good; k.n_used = n; REFUSED(sarx_tdbp_pair_check(2, &k), "n_used"); }
    { sarx_tdbp_pair_params k = good; k.n_used = INT32_MAX; REFUSED(sarx_tdbp_pair_check(2, &k), "outside"); }
    { sarx_tdbp_pair_params k = good; k.first_pulse[0] = INT32_MAX; REFUSED(sarx_tdbp_pair_check(2, &k), "outside"); }
    for (int ch = 0; ch < 2; ++ch) { sarx_tdbp_pair_params k = good; k.first_pulse[ch] = -1; REFUSED(sarx_tdbp_pair_check(2, &k), "first_pulse"); }

    const entry_fn entries[2] = {sarx_tdbp_pair_dev, sarx_tdbp_pair_host};
    for (sarx_tdbp_plan* plan : {(sarx_tdbp_plan*)nullptr, stale})
        for (entry_fn f : entries) {
            // NULL pointers, one at a time (either output alone may be NULL)
            REFUSED(f(plan, nullptr, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raw0, nullptr, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raw0, raw1, nullptr, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, nullptr, tp, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, nullptr, 0.0, vf, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, nullptr, 10.0, &good, img128, img64), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, nullptr, img128, img64), "NULL");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, nullptr, nullptr), "both outputs");
            // misaligned outputs
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, img128 + 8, img64), "misaligned");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64 + 4), "misaligned");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, nullptr, img64 + 1), "misaligned");
            // non-finite focus velocity, offsets and chirp centre
            for (double bad : {nan, inf, -inf}) {
                for (int i = 0; i < 3; ++i) {
                    vf[i] = bad;
                    REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, img128, nullptr), "vel_focus");
                    vf[i] = 0.0;
                }
                sarx_tdbp_pair_params k = good;
                k.rx_offset_m[1] = bad; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &k, nullptr, img64), "rx_offset_m");
                k = good; k.chirp_centre_s = bad; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &k, nullptr, img64), "chirp_centre_s");
            }
            // scene size
            for (double bad : {0.0, -1.0, nan, inf}) REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, bad, &good, img128, img64), "scene_size");
            // pulse ranges, as far as they can be judged without the plan's pulse count
            { sarx_tdbp_pair_params k = good; k.n_used = 0; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &k, img128, img64), "n_used"); }
            { sarx_tdbp_pair_params k = good; k.first_pulse[1] = -3; REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &k, img128, img64), "first_pulse"); }
            // everything else in order: the plan itself
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, img128, img64), "plan");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, nullptr, img64), "plan");
            REFUSED(f(plan, raw0, raw1, pos, vel, tp, 0.0, vf, 10.0, &good, img128, nullptr), "plan");
        }
    for (sarx_tdbp_plan* plan : {(sarx_tdbp_plan*)nullptr, stale}) {
        int tile = 7;
        REFUSED(sarx_tdbp_pair_route(plan, nullptr), "NULL");
        REFUSED(sarx_tdbp_pair_route(plan, &tile), "plan");
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
    if (failures) { fprintf(stderr, "tdbppair_asan_test: %d failures\n", failures); return 1; }
    printf("tdbppair_asan_test: all checks passed\n");
    return 0;
}
