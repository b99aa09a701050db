// Host-side sanitizer test of the ground relocation's entry points (include/sarx_relocate.h; `make asan-relocate` in csrc/,
// tests/test_relocate.py).
//
// Linked against the same libsarx_asan.so as abi_asan_test.cpp.  Runs where there is no GPU, so no context can exist: the
// parameter block is refused field by field with the field's name in sarx_last_error(NULL), and the device entry point is called
// without a context with the arguments a careless caller would pass - each pointer NULL in turn, bad and huge strides, misaligned
// and overlapping buffers, a bad parameter block - and must refuse every one before it reads a byte of them.  Every call returns
// SARX_ERR_INVALID with its message, never crashes.  Exit code 0 and no sanitizer report = pass.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../include/sarx_relocate.h"

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

static sarx_relocate_params good() {
    sarx_relocate_params p = {{0.0, -4000.0, 3000.0}, {100.0, 0.0, 0.0}, -180.0, -180.0, 4.0, 5.0, -1000.0, -1000.0, 2.0, 2.0, 1000, 1000, 8, 0};
    return p;
}

int main() {
    CHECK(sizeof(sarx_relocate_params) == 128 && sizeof(sarx_relocate_record) == 64);
    CHECK(offsetof(sarx_relocate_params, vel_ref) == 24 && offsetof(sarx_relocate_params, in_x0) == 48);
    CHECK(offsetof(sarx_relocate_params, out_x0) == 80 && offsetof(sarx_relocate_params, out_nx) == 112);
    CHECK(offsetof(sarx_relocate_params, max_detections) == 120 && offsetof(sarx_relocate_params, reserved) == 124);
    CHECK(offsetof(sarx_relocate_record, shift_x) == 16 && offsetof(sarx_relocate_record, vx) == 32);
    CHECK(offsetof(sarx_relocate_record, rank) == 48 && offsetof(sarx_relocate_record, status) == 52 && offsetof(sarx_relocate_record, flags) == 56);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    // the parameter block alone
    sarx_relocate_params p = good();
    CHECK(sarx_relocate_check(&p) == SARX_OK);
    p.out_nx = p.out_ny = SARX_TDBP_MULTI_MAX_DIM; p.max_detections = SARX_TDBP_MULTI_MAX_DETECTIONS; p.in_dx = -1e-300; p.out_dy = -3.0;
    p.vel_ref[0] = p.vel_ref[1] = 0.0;                                 // no track direction: a status per report, not a refusal
    CHECK(sarx_relocate_check(&p) == SARX_OK);
    p = good(); p.out_nx = p.out_ny = p.max_detections = 1;
    CHECK(sarx_relocate_check(&p) == SARX_OK);
    REFUSED(sarx_relocate_check(nullptr), "NULL");
    for (double bad : {nan, inf, -inf}) {
        for (int k = 0; k < 3; ++k) {
            char word[16];
            p = good(); p.pos_ref[k] = bad; snprintf(word, sizeof word, "pos_ref[%d]", k); REFUSED(sarx_relocate_check(&p), word);
            p = good(); p.vel_ref[k] = bad; snprintf(word, sizeof word, "vel_ref[%d]", k); REFUSED(sarx_relocate_check(&p), word);
        }
        p = good(); p.in_x0 = bad; REFUSED(sarx_relocate_check(&p), "in_x0");
        p = good(); p.in_y0 = bad; REFUSED(sarx_relocate_check(&p), "in_y0");
        p = good(); p.in_dx = bad; REFUSED(sarx_relocate_check(&p), "in_dx");
        p = good(); p.in_dy = bad; REFUSED(sarx_relocate_check(&p), "in_dy");
        p = good(); p.out_x0 = bad; REFUSED(sarx_relocate_check(&p), "out_x0");
        p = good(); p.out_y0 = bad; REFUSED(sarx_relocate_check(&p), "out_y0");
        p = good(); p.out_dx = bad; REFUSED(sarx_relocate_check(&p), "out_dx");
        p = good(); p.out_dy = bad; REFUSED(sarx_relocate_check(&p), "out_dy");
    }
    for (double zero : {0.0, -0.0}) {
        p = good(); p.in_dx = zero; REFUSED(sarx_relocate_check(&p), "in_dx");
        p = good(); p.in_dy = zero; REFUSED(sarx_relocate_check(&p), "in_dy");
        p = good(); p.out_dx = zero; REFUSED(sarx_relocate_check(&p), "out_dx");
        p = good(); p.out_dy = zero; REFUSED(sarx_relocate_check(&p), "out_dy");
    }
    for (int n : {0, -1, SARX_TDBP_MULTI_MAX_DIM + 1, INT32_MAX, INT32_MIN}) {
        p = good(); p.out_nx = n; REFUSED(sarx_relocate_check(&p), "out_nx");
        p = good(); p.out_ny = n; REFUSED(sarx_relocate_check(&p), "out_ny");
    }
    for (int md : {0, -1, SARX_TDBP_MULTI_MAX_DETECTIONS + 1, INT32_MAX, INT32_MIN}) {
        p = good(); p.max_detections = md; REFUSED(sarx_relocate_check(&p), "max_detections");
    }
    for (int r : {1, -1}) { p = good(); p.reserved = r; REFUSED(sarx_relocate_check(&p), "reserved"); }

    // the device entry point without a context: nothing behind the pointers is read, whatever they are
    p = good();                                                        // slot 16 + 48 * 8 = 400 bytes, records 512
    alignas(16) static char buf[8192];
    char* in = buf; char* v = buf + 512; char* valid = buf + 1024; char* along = buf + 1536; char* rec = buf + 2048; char* out = buf + 4096;
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, rec, out), "ctx");
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, nullptr, 0, nullptr, 0, rec, out), "ctx");
    REFUSED(sarx_relocate_dev(nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr), "ctx");
    REFUSED(sarx_relocate_dev(nullptr, &p, nullptr, v, 8, valid, 4, along, 8, rec, out), "ctx");
    REFUSED(sarx_relocate_dev(nullptr, &p, in, nullptr, 8, valid, 4, along, 8, rec, out), "ctx");
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, nullptr, out), "ctx");
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, rec, nullptr), "ctx");
    for (size_t s : {(size_t)0, (size_t)4, (size_t)12, (size_t)63, SIZE_MAX, SIZE_MAX - 7}) {          // strides
        REFUSED(sarx_relocate_dev(nullptr, &p, in, v, s, valid, 4, along, 8, rec, out), "ctx");
        REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, s, along, 8, rec, out), "ctx");
        REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, s, rec, out), "ctx");
    }
    REFUSED(sarx_relocate_dev(nullptr, &p, in + 4, v, 8, valid, 4, along, 8, rec, out), "ctx");        // misaligned
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v + 4, 8, valid + 2, 4, along + 1, 8, rec + 4, out + 4), "ctx");
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, rec, in), "ctx");             // in place
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, in + 392, out), "ctx");       // records over the input slot
    REFUSED(sarx_relocate_dev(nullptr, &p, in, rec, 64, rec + 60, 64, along, 8, rec, out), "ctx");     // the speeds inside the records
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, rec, rec + 16), "ctx");       // the two outputs
    for (int md : {0, -1, INT32_MAX}) {
        p = good(); p.max_detections = md;
        REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, rec, out), "ctx");
    }
    p = good(); p.in_dx = nan;
    REFUSED(sarx_relocate_dev(nullptr, &p, in, v, 8, valid, 4, along, 8, rec, out), "ctx");

    sarx_ctx* ctx = nullptr;
    if (sarx_init(0, &ctx) == SARX_OK) {
        sarx_destroy(ctx);                                             // a box with a device: nothing more to check here
    } else {
        CHECK(ctx == nullptr);
        CHECK(strlen(sarx_last_error(nullptr)) > 5);
    }
    if (failures) { fprintf(stderr, "relocate_asan_test: %d failures\n", failures); return 1; }
    printf("relocate_asan_test: all checks passed\n");
    return 0;
}
