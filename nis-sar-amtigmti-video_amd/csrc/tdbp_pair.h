// Two-receiver back-projection: both channels of one CPI onto one ground grid in one launch, the N = 2 case of tdbp_multi.h; see tdbp_pair.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sarx_tdbp_pair.h"
#include "tdbp_multi.h"

namespace sarx {
// raw0, raw1: device [n_p][n_s]; pos, vel: host [n_p][3] (no zero vel row); t_pulses: host [n_p]; vel_focus: host [3]; prm: checked
// by the caller against n_p.  chunks: pulse chunks, 0 = chosen here.  d_img128: device complex128 [2][ny][nx] or NULL; d_img64: device
// complex64 [2][ny][nx] or NULL.
hipError_t tdbp_pair(Tdbp* t, const float2* raw0, const float2* raw1, const double* pos, const double* vel, const double* t_pulses,
                     double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_pair_params* prm, int chunks,
                     double2* d_img128, float2* d_img64, hipStream_t st);
int tdbp_pair_route(const Tdbp* t);                     // 1 tile form, 0 exact form, -1 no pair call yet
// device staging of the host entry point: the second channel's raw pulses [n_p][n_s] and both output forms
hipError_t tdbp_pair_staging(Tdbp* t, float2** d_raw1, double2** d_img128, float2** d_img64);
// the stack's parameter block of the pair: n_rx = 2, the unused slots 0
inline sarx_tdbp_multi_params tdbp_pair_as_multi(const sarx_tdbp_pair_params& k) {
    sarx_tdbp_multi_params m{};
    for (int c = 0; c < 2; ++c) { m.rx_offset_m[c] = k.rx_offset_m[c]; m.first_pulse[c] = k.first_pulse[c]; }
    m.chirp_centre_s = k.chirp_centre_s; m.n_used = k.n_used; m.n_rx = 2;
    return m;
}
}  // namespace sarx
