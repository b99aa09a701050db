// Internal launch interface of the GMTI ATI gate (atigate.hip) for the C ABI (api_atigate.hip, include/sarx_atigate.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_atigate.h"

static_assert(sizeof(sarx_atigate_params) == 64, "sarx_atigate_params is 64 bytes");
static_assert(sizeof(sarx_atigate_stat) == 96, "sarx_atigate_stat is 96 bytes");
static_assert(sizeof(sarx_gmti_report) == 48 && sizeof(sarx_gmti_header) == 16, "the GMTI slot layout");

namespace sarx {

struct AtiGateArgs {
    sarx_atigate_params p;
    const float2* a;                       // slc1, [n_az x n_rg]
    const float2* b;                       // slc2
    int n_az, n_rg;
    const char* in;                        // the input slot
    char* out;                             // the output slot
    sarx_atigate_stat* stats;              // or NULL
    int32_t* keep;                         // SARX_ATIGATE_MAX_DETECTIONS flags: the statistics launch writes them, the compaction reads them
};
// the statistics launch (one workgroup per report) and the compaction launch (one workgroup)
hipError_t launch_atigate(const AtiGateArgs& a, hipStream_t st);

}  // namespace sarx
