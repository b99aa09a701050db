// Internal launch interface of the Kalman ground tracker (ktrack.hip) for the C ABI (api_ktrack.hip, include/sarx_ktrack.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_ktrack.h"

static_assert(sizeof(sarx_ktrack_params) == 80, "sarx_ktrack_params is 80 bytes");
static_assert(sizeof(sarx_ktrack_frame) == 64, "sarx_ktrack_frame is 64 bytes");
static_assert(sizeof(sarx_ktrack_header) == 64, "sarx_ktrack_header is 64 bytes");
static_assert(sizeof(sarx_ktrack_slot) == 192, "sarx_ktrack_slot is 192 bytes");

namespace sarx {

constexpr int KTRACK_STAGE = 256;          // entries per LDS stage of the pair launch; the arrays below are padded to it
constexpr int KTRACK_PRED = 14;            // doubles per predicted track: x-, y-, vx-, vy-, P-[10]
constexpr int KTRACK_MEAS = 11;            // doubles per measurement: z[3], u[2], Rm00 Rm01 Rm11 Rm02 Rm12 Rm22

// workspace: pred[KTRACK_PRED][tp], nis[tp], meas[KTRACK_MEAS][rp] (fp64, one plane per value), best_r[tp], best_t[rp],
// free_slot[tp] (int32), tp and rp = the capacities rounded up to KTRACK_STAGE
inline size_t ktrack_padded(int n) { return ((size_t)n + KTRACK_STAGE - 1) / KTRACK_STAGE * KTRACK_STAGE; }
inline size_t ktrack_workspace_bytes(int max_tracks, int max_det) {
    const size_t tp = ktrack_padded(max_tracks), rp = ktrack_padded(max_det);
    return ((KTRACK_PRED + 1) * tp + KTRACK_MEAS * rp) * sizeof(double) + (2 * tp + rp) * sizeof(int32_t);
}

struct KtrackArgs {
    sarx_ktrack_params p;
    sarx_ktrack_frame f;
    const sarx_gmti_header* slot_hdr;
    const sarx_gmti_report* rep;
    const sarx_relocate_record* rec;
    const char* v_los;
    size_t v_los_stride;
    sarx_ktrack_header* hdr;
    sarx_ktrack_slot* slots;
    int32_t* assoc;                        // or NULL
    double* pred;                          // [KTRACK_PRED][tp]
    double* nis;                           // [tp]: d2 of a matched track
    double* meas;                          // [KTRACK_MEAS][rp]
    int32_t* best_r;                       // [tp]
    int32_t* best_t;                       // [rp]
    int32_t* free_slot;                    // [tp]
    int tp, rp;
};
hipError_t launch_ktrack_init(sarx_ktrack_header* hdr, sarx_ktrack_slot* slots, int max_tracks, hipStream_t st);
hipError_t launch_ktrack_step(const KtrackArgs& a, hipStream_t st);

}  // namespace sarx
