// Two-receiver back-projection: both channels of one CPI onto one ground grid in one launch; see tdbp_pair.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sarx_tdbp_pair.h"
#include "tdbp.h"

namespace sarx {
struct TdbpPair;                                        // the pair's scratch, owned by the plan
// raw0, raw1: device [n_p][n_s]; pos, vel: host [n_p][3] (no zero vel row); t_pulses: host [n_p]; vel_focus: host [3]; prm: checked
// by the caller against n_p.  chunks: pulse chunks, 0 = chosen here.  d_img128: device complex128 [2][ny][nx] or NULL; d_img64: device
// complex64 [2][ny][nx] or NULL.
hipError_t tdbp_pair(Tdbp* t, const float2* raw0, const float2* raw1, const double* pos, const double* vel, const double* t_pulses,
                     double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_pair_params* prm, int chunks,
                     double2* d_img128, float2* d_img64, hipStream_t st);
int tdbp_pair_route(const Tdbp* t);                     // 1 tile form, 0 exact form, -1 no pair call yet
// device staging of the host entry point: the second channel's raw pulses [n_p][n_s] and both output forms
hipError_t tdbp_pair_staging(Tdbp* t, float2** d_raw1, double2** d_img128, float2** d_img64);
void tdbp_pair_free(TdbpPair* s);
}  // namespace sarx
