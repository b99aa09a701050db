// Internal launch interface of the sliding-window coherence (coherence.hip) for the C ABI (api_coherence.hip, include/sarx_coherence.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_coherence.h"

static_assert(sizeof(sarx_coherence_params) == 32, "sarx_coherence_params is 32 bytes");
static_assert(sizeof(sarx_coherence_summary) == 64, "sarx_coherence_summary is 64 bytes");

namespace sarx {

constexpr int COH_TH = 64;                 // output rows of a workgroup's tile
constexpr int COH_TW = 224;                // output columns of it: 32 segments of 7

struct CohPartial {                        // one workgroup's share of the summary in the workspace
    unsigned long long n_tested, n_changed;
    double sum_coh;
};

struct CoherenceArgs {
    const float2* a;
    const float2* b;
    int n_az, n_rg, ha, hr;
    float threshold;                       // (float)params.threshold
    double power_floor;
    float* coh;
    float2* igram;                         // or NULL
    uint8_t* mask;                         // or NULL
    sarx_coherence_summary* summary;       // or NULL
    CohPartial* part;                      // [tiles]: needed with summary
};
inline unsigned coherence_tiles_rg(int n_rg) { return (unsigned)((n_rg + COH_TW - 1) / COH_TW); }
inline unsigned coherence_tiles_az(int n_az) { return (unsigned)((n_az + COH_TH - 1) / COH_TH); }
hipError_t launch_coherence(const CoherenceArgs& a, hipStream_t st);

}  // namespace sarx
