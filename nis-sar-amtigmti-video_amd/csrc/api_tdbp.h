// The refusals that api_tdbp_search.hip, api_tdbp_pair.hip, api_tdbp_pair_search.hip and api_tdbp_multi.hip have in common, each message
// stated once.
// c: where the message goes (NULL: the caller has no live plan, sarx_last_error(NULL) gets it).
#pragma once
#include "../../include/sarx_tdbp_pair.h"
#include "api_ctx.h"

#include <cmath>

namespace sarx {

// what can be said of the pair's parameter block alone; n_pulses < 0: the pulse count is not known yet, the upper end is checked later
inline int tdbp_pair_params_check(sarx_ctx* c, int n_pulses, const sarx_tdbp_pair_params* k) {
    if (!k) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (!std::isfinite(k->rx_offset_m[0]) || !std::isfinite(k->rx_offset_m[1])) return fail(c, SARX_ERR_INVALID, "rx_offset_m must be finite");
    if (!std::isfinite(k->chirp_centre_s)) return fail(c, SARX_ERR_INVALID, "chirp_centre_s must be finite");
    if (k->n_used < 1) return fail(c, SARX_ERR_INVALID, "n_used %d must be >= 1", k->n_used);
    for (int ch = 0; ch < 2; ++ch) {
        if (k->first_pulse[ch] < 0) return fail(c, SARX_ERR_INVALID, "first_pulse[%d] = %d must be >= 0", ch, k->first_pulse[ch]);
        if (n_pulses >= 0 && (long long)k->first_pulse[ch] + k->n_used > n_pulses)
            return fail(c, SARX_ERR_INVALID, "channel %d: pulses %d .. %lld lie outside [0, %d]", ch, k->first_pulse[ch],
                        (long long)k->first_pulse[ch] + k->n_used, n_pulses);
    }
    return SARX_OK;
}
// vel_tx [n_p][3]: the pair divides by every row's length
inline int tdbp_vel_tx_check(sarx_ctx* c, const double* vel_tx, int n_p) {
    for (int i = 0; i < n_p; ++i) {
        const double v2 = vel_tx[3 * i] * vel_tx[3 * i] + vel_tx[3 * i + 1] * vel_tx[3 * i + 1] + vel_tx[3 * i + 2] * vel_tx[3 * i + 2];
        if (!(v2 > 0 && std::isfinite(v2))) return fail(c, SARX_ERR_INVALID, "vel_tx row %d is zero or not finite", i);
    }
    return SARX_OK;
}
// vel_hyps [n_hyp][3] of a search
inline int tdbp_hyps_check(sarx_ctx* c, const double* vel_hyps, int n_hyp) {
    for (int i = 0; i < 3 * n_hyp; ++i)
        if (!std::isfinite(vel_hyps[i])) return fail(c, SARX_ERR_INVALID, "focus velocity %d has a non-finite component", i / 3);
    return SARX_OK;
}
inline int tdbp_scene_check(sarx_ctx* c, double scene_size) {
    return scene_size > 0 && std::isfinite(scene_size) ? (int)SARX_OK : fail(c, SARX_ERR_INVALID, "scene_size must be positive");
}
// sarx_tdbp_*_route: route is the unit's own query (1 tile form, 0 exact form, -1 no call yet), not_yet what is said of -1
inline int tdbp_route_query(const sarx_tdbp_plan* p, int (*route)(const Tdbp*), const char* not_yet, int* tile) {
    if (!tile) return fail(nullptr, SARX_ERR_INVALID, "NULL pointer");
    sarx_ctx* c = nullptr;
    if (const int rc = tdbp_plan_usable(p, &c)) return rc;
    const int r = route(p->t);
    if (r < 0) return fail(c, SARX_ERR_INVALID, "%s", not_yet);
    *tile = r;
    return SARX_OK;
}

}  // namespace sarx
