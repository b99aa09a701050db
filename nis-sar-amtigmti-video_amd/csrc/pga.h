// Internal launch interface of the phase-gradient autofocus (pga.hip) for the C ABI (api_pga.hip, include/sarx_pga.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_pga.h"

static_assert(sizeof(sarx_pga_params) == 56, "sarx_pga_params is 56 bytes");
static_assert(sizeof(sarx_pga_record) == 32, "sarx_pga_record is 32 bytes");

namespace sarx {

// columns per tile: L x WT = 4096 points, 256 threads and 32 KiB of LDS for every L
constexpr int pga_tile_cols(int L) { return 4096 / L; }
inline int pga_tiles(int L, int n_rg) { return (n_rg + pga_tile_cols(L) - 1) / pga_tile_cols(L); }
// workspace: per frame and tile one row of 3 L + 4 doubles: P[L], Re S[L], Im S[L], then s2, s4, the used columns, 0
constexpr size_t pga_row_doubles(int L) { return 3 * (size_t)L + 4; }

struct PgaLayout {
    int L, n_rg, n_frames;
    size_t ld, frame_stride;           // in elements
};

struct PgaEstimateArgs {
    PgaLayout g;
    const float2* src;                 // g_it
    int half_width;
    double min_contrast, power_floor;
    double* work;                      // [n_frames x tiles x (3 L + 4)]
    double* phase;                     // phi_tot [n_frames x L]
    sarx_pga_record* rec;              // this estimate's record of frame 0; frame f's lies rec_stride records on
    int rec_stride;
    int first;                         // phi_tot = phi (the first estimate), else phi_tot += phi
    int update;                        // 0: the final estimate, phi_tot is left alone
};
struct PgaApplyArgs {
    PgaLayout g;
    const float2* src;
    float2* dst;
    const double* phase;
    size_t phase_stride;
    double sign_rev;                   // sign / (2 pi): radians to revolutions
};

hipError_t launch_pga_estimate(const PgaEstimateArgs& a, hipStream_t st);      // the estimate launch and the integrate launch
hipError_t launch_pga_apply(const PgaApplyArgs& a, hipStream_t st);

}  // namespace sarx
