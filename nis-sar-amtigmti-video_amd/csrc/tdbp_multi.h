// N-receiver back-projection and the multi-baseline ATI resolver; see tdbp_multi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sarx_tdbp_multi.h"
#include "tdbp.h"

namespace sarx {
struct TdbpRx;                                          // the scratch of a receiver stack (tdbp_plan.h), owned by the plan
// raw: n_rx device pointers [n_p][n_s]; pos, vel: host [n_p][3] (no zero vel row); t_pulses: host [n_p]; vel_focus: host [3]; prm:
// checked by the caller against n_p.  chunks: pulse chunks, 0 = chosen here.  d_img128: device complex128 [n_rx][ny][nx] or NULL;
// d_img64: device complex64 [n_rx][ny][nx] or NULL.
hipError_t tdbp_multi(Tdbp* t, const float2* const* raw, const double* pos, const double* vel, const double* t_pulses, double t_start,
                      const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* prm, int chunks, double2* d_img128,
                      float2* d_img64, hipStream_t st);
int tdbp_multi_route(const Tdbp* t);                    // 1 tile form, 0 exact form, -1 no multi call yet
// device staging of the host entry point: the raw pulses of channels 1 .. n_rx - 1 [n_p][n_s] and both output forms [n_rx][ny][nx]
hipError_t tdbp_multi_staging(Tdbp* t, int n_rx, float2** d_raw, double2** d_img128, float2** d_img64);
// bytes the scratch holds on the device and a sum over its buffers' addresses (0, 0 before any multi call)
void tdbp_multi_held(const Tdbp* t, uint64_t* bytes, uint64_t* id);

struct MultiResolveArgs {
    sarx_tdbp_multi_resolve_params p;
    const float2* imgs;      // [n_rx][ny][nx]
    const char* slot;        // sarx_gmti_header, then max_detections sarx_gmti_report
    sarx_tdbp_multi_record* rec;
    int ny, nx;
};
hipError_t launch_multi_resolve(const MultiResolveArgs& a, hipStream_t st);
}  // namespace sarx
