// Focus-velocity search on the two-receiver back-projection, per GMTI report; see tdbp_pair_search.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/sarx_tdbp_pair_search.h"
#include "tdbp.h"

namespace sarx {
struct TdbpPairSearch;                                  // the scratch, owned by the plan
// raw0, raw1: device [n_p][n_s]; pos, vel: host [n_p][3] (no zero vel row); t_pulses: host [n_p]; prm, sp: checked by the caller
// against n_p and the grid; vel_hyps: host [sp->n_hyp][3], finite.  d_reports, d_header: the device slot of max_det reports.
// chunks: pulse chunks, 0 = chosen here.  d_records [max_det][n_hyp], d_best [max_det], d_chips [max_det][n_hyp][2][chip_y][chip_x] or NULL.
// hipErrorInvalidValue with *why set: the partial sums do not fit (nothing was enqueued).
hipError_t tdbp_pair_search(Tdbp* t, const float2* raw0, const float2* raw1, const double* pos, const double* vel, const double* t_pulses,
                            double t_start, double scene_size, const sarx_tdbp_pair_params* prm, const double* vel_hyps,
                            const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_det,
                            const sarx_tdbp_pair_search_params* sp, int chunks, sarx_tdbp_search_record* d_records,
                            sarx_tdbp_pair_search_best* d_best, double2* d_chips, std::string* why, hipStream_t st);
int tdbp_pair_search_route(const Tdbp* t);              // 1 tile form, 0 exact form, -1 no call yet
// device staging of the host entry point, grown on demand: the second channel's raw pulses, the slot, and the three outputs
struct PairSearchStaging {
    float2* raw1;
    void* slot;
    sarx_tdbp_search_record* rec;
    sarx_tdbp_pair_search_best* best;
    double2* chips;                                     // NULL unless asked for
};
hipError_t tdbp_pair_search_staging(Tdbp* t, int max_det, const sarx_tdbp_pair_search_params* sp, bool chips, PairSearchStaging* out);
void tdbp_pair_search_free(TdbpPairSearch* s);
}  // namespace sarx
