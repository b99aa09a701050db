// Time-domain back-projection (sar_batch_sim.py:171-238); see tdbp.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/sarx.h"

namespace sarx {
struct Tdbp;
Tdbp* tdbp_create(int n_pulses, int num_samples, int nx, int ny, const sarx_tdbp_params* k, const float2* tw_all, std::string& err);
void tdbp_destroy(Tdbp* t);
hipError_t tdbp_focus(Tdbp* t, const float2* raw_dev, const double* pos, const double* vel, const double* t_pulses, double t_start,
                      const double* vel_focus, double scene_size, bool all_samples, hipStream_t st);
void tdbp_window(const Tdbp* t, int* lo, int* hi);   // samples range-compressed by the last call
const double2* tdbp_image(const Tdbp* t);     // device, complex128 [ny][nx]
const float2* tdbp_rc(const Tdbp* t);         // device, complex64 [n_pulses][num_samples]
uint64_t tdbp_bytes(const Tdbp* t);

// ---- what the focus-velocity search (tdbp_search.hip) needs of a plan ----
struct PulseGeo {            // one 64-byte record per pulse, read with scalar loads
    double px, py, pz;       // platform position
    double wx, wy, wz;       // platform velocity - focus velocity  (v_rel, :211)
    double dt, pad;          // t_pulse - mean(t_pulses) (:203-204); pad = |v_rel|^2
};
struct TdbpView {
    int n_p, n_s, nx, ny;
    sarx_tdbp_params k;
    const float2* rc;        // [n_p][n_s], filled by tdbp_range_compress
    const double *xax, *yax; // pixel axes, valid after tdbp_ensure_axes
    bool full_rc;
};
struct TdbpSearch;
TdbpView tdbp_view(const Tdbp* t);
TdbpSearch*& tdbp_search_slot(Tdbp* t);       // the search's scratch, owned by the plan (freed by tdbp_destroy)
hipError_t tdbp_range_compress(Tdbp* t, const float2* raw, int lo, int hi, hipStream_t st);
hipError_t tdbp_ensure_axes(Tdbp* t, double scene_size, hipStream_t st);
// geo holds w = v_plat - vf for the SAME vf
void tdbp_sample_window(const Tdbp* t, const std::vector<PulseGeo>& geo, const double* vf, double t_start, double scene_size,
                        int* lo, int* hi);
bool tdbp_tile_ok(const Tdbp* t, const std::vector<PulseGeo>& geo, const double* vf, double scene_size);
}  // namespace sarx
