// Internal launch interface of the GMTI detector (gmti.hip) for the C ABI (api_gmti.hip, include/sarx_gmti.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_gmti.h"

namespace sarx {

struct GmtiCfarArgs {
    const float* m;              // DPCA magnitude plane [n_az x n_rg]
    int n_az, n_rg;
    int ga, gr;                  // guard half-widths
    int oa, orr;                 // outer half-widths (guard + train), <= SARX_GMTI_MAX_HALF
    double alpha;
    int min_train, max_det;
    sarx_gmti_report* rep;
    sarx_gmti_header* hdr;       // zeroed on the stream before the launch
};
hipError_t launch_gmti_cfar(const GmtiCfarArgs& a, hipStream_t st);

// src: the CFAR launch's unordered list (a copy: dst is written in sorted order), dst: the caller's list
hipError_t launch_gmti_refine(const float2* s1, const float2* s2, int n_az, int n_rg, double cal_phase, const sarx_gmti_report* src,
                              sarx_gmti_report* dst, const sarx_gmti_header* hdr, int max_det, hipStream_t st);

}  // namespace sarx
