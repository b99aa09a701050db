// Focus-velocity search of the back-projection: many hypotheses of one CPI in one enqueue; see tdbp_search.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sarx_tdbp_search.h"
#include "tdbp.h"

namespace sarx {
struct TdbpSearch;                                      // the search's scratch, owned by the plan
// raw: device [n_p][n_s]; pos, vel: host [n_p][3]; t_pulses: host [n_p]; vel_hyps: host [n_hyp][3] (finite, 1 <= n_hyp <= MAX_HYP: the
// caller checked).  d_images: device complex128 [n_hyp][ny][nx] or NULL; d_records: device [n_hyp].  chunks: pulse chunks, 0 = chosen here.
hipError_t tdbp_search(Tdbp* t, const float2* raw, const double* pos, const double* vel, const double* t_pulses, double t_start,
                       const double* vel_hyps, int n_hyp, double scene_size, int chunks, double2* d_images,
                       sarx_tdbp_search_record* d_records, hipStream_t st);
// the metric launch alone over a stack [n_hyp][ny][nx] the caller holds
hipError_t tdbp_search_metric(Tdbp* t, const double2* d_stack, int n_hyp, sarx_tdbp_search_record* d_records, hipStream_t st);
int tdbp_search_route(const Tdbp* t);                   // 1 tile form, 0 exact form, -1 no search yet
// device staging of the host entry point: records [MAX_HYP] always, a stack of n_hyp images when asked (grown on demand)
hipError_t tdbp_search_staging(Tdbp* t, int n_hyp, bool images, sarx_tdbp_search_record** d_records, double2** d_images, hipStream_t st);
void tdbp_search_free(TdbpSearch* s);
}  // namespace sarx
