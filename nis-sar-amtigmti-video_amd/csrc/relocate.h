// Ground relocation of GMTI reports; see relocate.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sarx_relocate.h"

namespace sarx {
struct RelocateArgs {
    sarx_relocate_params p;
    const char* in;                 // sarx_gmti_header, then max_detections sarx_gmti_report
    const char* v_los;              // fp64 per report, v_los_stride bytes apart
    const char* valid;              // uint32 per report, valid_stride apart, or NULL
    const char* v_along;            // fp64 per report, v_along_stride apart, or NULL
    size_t v_los_stride, valid_stride, v_along_stride;
    sarx_relocate_record* rec;      // max_detections records
    char* out;                      // the output slot
    long long* keys;                // max_detections sort keys between the two launches (the lane's scratch)
};
hipError_t launch_relocate(const RelocateArgs& a, hipStream_t st);
}  // namespace sarx
