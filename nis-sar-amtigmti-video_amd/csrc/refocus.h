// Internal launch interface of the GMTI refocus (refocus.hip) for the C ABI (api_gmti.hip, include/sarx_refocus.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_refocus.h"

static_assert(sizeof(sarx_refocus_record) == 48, "sarx_refocus_record is 48 bytes");
static_assert(sizeof(sarx_refocus_params) == 576, "sarx_refocus_params is 576 bytes");

namespace sarx {

struct RefocusArgs {
    const float2* s1;
    const float2* s2;                  // SLC1 source: slc1 again, weighted by zero
    float2 w2;                         // x = s1 - w2 * s2: e^{j cal} (DPCA) or 0 (SLC1)
    int n_az, n_rg;
    int L, W, n_hyp;
    double lam, vr, prf, r0, dr;
    const sarx_gmti_report* rep;
    const sarx_gmti_header* hdr;
    int max_det;
    float* curves;                     // [max_det x n_hyp], never NULL (a ctx scratch buffer when the caller wants none)
    sarx_refocus_record* rec;
    float2* chips;                     // [max_det x L x W] or NULL
    double vp[SARX_REFOCUS_MAX_HYP];
};
hipError_t launch_refocus(const RefocusArgs& a, hipStream_t st);

}  // namespace sarx
