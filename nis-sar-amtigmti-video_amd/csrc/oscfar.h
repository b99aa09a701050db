// Internal launch interface of the ordered-statistic CFAR (oscfar.hip) for the C ABI (api_oscfar.hip, include/sarx_oscfar.h).
#pragma once
#include "gmti.h"

#include "../../include/sarx_oscfar.h"

namespace sarx {

struct OsCfarArgs {
    GmtiCfarArgs base;           // plane, half-widths, alpha, min_train, max_det, report list and header, as the CA launch takes them
    int rank, n_full;            // 1 <= rank <= n_full = training cells of a window wholly inside the image
};
hipError_t launch_gmti_oscfar(const OsCfarArgs& a, hipStream_t st);

}  // namespace sarx
