// Internal launch interface of the GMTI plot extraction (cluster.hip) for the C ABI (api_cluster.hip, include/sarx_cluster.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_cluster.h"

static_assert(sizeof(sarx_cluster_params) == 16, "sarx_cluster_params is 16 bytes");
static_assert(sizeof(sarx_cluster_plot) == 64, "sarx_cluster_plot is 64 bytes");
static_assert(sizeof(sarx_gmti_report) == 48 && sizeof(sarx_gmti_header) == 16, "the GMTI slot layout");

namespace sarx {

struct ClusterArgs {
    sarx_cluster_params p;
    const char* in;                        // frame f's slot at in + f * in_stride
    char* out;
    char* plots;                           // or NULL
    int32_t* labels;                       // or NULL; frame f's row at labels + f * max_detections
    size_t in_stride, out_stride, plots_stride;
};
// one workgroup per frame; n_frames >= 1
hipError_t launch_cluster(const ClusterArgs& a, int n_frames, hipStream_t st);

}  // namespace sarx
