// Internal launch interface of the two-channel balance (balance.hip) for the C ABI (api_balance.hip, include/sarx_balance.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_balance.h"

static_assert(sizeof(sarx_balance_header) == 64, "sarx_balance_header is 64 bytes");
static_assert(sizeof(sarx_balance_record) == 64, "sarx_balance_record is 64 bytes");
static_assert(sizeof(sarx_balance_params) == 40, "sarx_balance_params is 40 bytes");

namespace sarx {

constexpr int BAL_STRIP_ROWS = 32;         // a block is cut into strips of this many rows, one workgroup each

struct BalPartial {                        // one strip's sums in the workspace
    double s12_re, s12_im, s11, s22;
    unsigned long long n;
};

struct BalanceGeom {
    int n_az, n_rg, block_az, block_rg, nb_az, nb_rg;
    int strips;                            // strips per block: ceil(block_az / BAL_STRIP_ROWS)
};
inline BalanceGeom balance_geom(int n_az, int n_rg, int block_az, int block_rg) {
    BalanceGeom g{n_az, n_rg, block_az, block_rg, (n_az + block_az - 1) / block_az, (n_rg + block_rg - 1) / block_rg, 0};
    g.strips = (block_az + BAL_STRIP_ROWS - 1) / BAL_STRIP_ROWS;
    return g;
}

struct BalanceEstimateArgs {
    const float2* s1;
    const float2* s2;
    BalanceGeom g;
    float clip;                            // (float)clip_power
    int mode, min_count;
    double min_coherence;
    BalPartial* part;                      // [nb_az nb_rg strips]
    sarx_balance_header* hdr;
    sarx_balance_record* rec;
};
hipError_t launch_balance_estimate(const BalanceEstimateArgs& a, hipStream_t st);

struct BalanceApplyArgs {
    const float2* s1;                      // NULL without dm
    const float2* s2;
    float2* out;                           // may be s2
    float* dm;                             // or NULL
    BalanceGeom g;
    int interp;
    const sarx_balance_record* rec;
};
hipError_t launch_balance_apply(const BalanceApplyArgs& a, hipStream_t st);

}  // namespace sarx
