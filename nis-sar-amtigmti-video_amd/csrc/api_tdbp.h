// The refusals that api_tdbp_search.hip, api_tdbp_pair.hip, api_tdbp_pair_search.hip and api_tdbp_multi.hip have in common, each message
// stated once; the pair's parameter block and calls are checked as the receiver stack's with two channels.
// c: where the message goes (NULL: the caller has no live plan, sarx_last_error(NULL) gets it).
#pragma once
#include "api_ctx.h"
#include "tdbp_pair.h"

#include <cmath>

namespace sarx {

// what can be said of the stack's parameter block alone; n_pulses < 0: the pulse count is not known yet, the upper end is checked later
inline int tdbp_multi_params_check(sarx_ctx* c, int n_pulses, const sarx_tdbp_multi_params* k) {
    if (!k) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (k->n_rx < 2 || k->n_rx > SARX_TDBP_MULTI_MAX_RX) return fail(c, SARX_ERR_INVALID, "n_rx %d must be 2 .. %d", k->n_rx, SARX_TDBP_MULTI_MAX_RX);
    for (int ch = 0; ch < k->n_rx; ++ch)
        if (!std::isfinite(k->rx_offset_m[ch])) return fail(c, SARX_ERR_INVALID, "rx_offset_m must be finite");
    for (int ch = k->n_rx; ch < SARX_TDBP_MULTI_MAX_RX; ++ch)
        if (!(k->rx_offset_m[ch] == 0.0) || k->first_pulse[ch] != 0)
            return fail(c, SARX_ERR_INVALID, "unused slot %d of rx_offset_m and first_pulse must be 0", ch);
    if (!std::isfinite(k->chirp_centre_s)) return fail(c, SARX_ERR_INVALID, "chirp_centre_s must be finite");
    if (k->n_used < 1) return fail(c, SARX_ERR_INVALID, "n_used %d must be >= 1", k->n_used);
    for (int ch = 0; ch < k->n_rx; ++ch) {
        if (k->first_pulse[ch] < 0) return fail(c, SARX_ERR_INVALID, "first_pulse[%d] = %d must be >= 0", ch, k->first_pulse[ch]);
        if (n_pulses >= 0 && (long long)k->first_pulse[ch] + k->n_used > n_pulses)
            return fail(c, SARX_ERR_INVALID, "channel %d: pulses %d .. %lld lie outside [0, %d]", ch, k->first_pulse[ch],
                        (long long)k->first_pulse[ch] + k->n_used, n_pulses);
    }
    return SARX_OK;
}
// the pair's parameter block: the stack's with n_rx = 2, whose own two refusals (n_rx, the unused slots) cannot then occur
inline int tdbp_pair_params_check(sarx_ctx* c, int n_pulses, const sarx_tdbp_pair_params* k) {
    if (!k) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    const sarx_tdbp_multi_params m = tdbp_pair_as_multi(*k);
    return tdbp_multi_params_check(c, n_pulses, &m);
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
// A call of sarx_tdbp_pair_* or sarx_tdbp_multi_*, the pair as the stack's parameter block and pointer list.  Everything that can be
// refused without reading the plan is refused first, so a caller without a device gets the same answers; the channel pointers are
// read only once n_rx is known to be good.  The plan next: NULL, or not (or no longer) one that sarx_tdbp_plan_create returned.  Last
// what needs the plan's pulse count: the upper end of the pulse ranges and the rows of vel_tx.  *c: where the message goes.
inline int tdbp_rx_check(sarx_tdbp_plan* p, bool pointers_ok, const void* const* raw, const double* vel_tx, const double* vel_focus,
                         double scene_size, const sarx_tdbp_multi_params* k, const void* img128, const void* img64, sarx_ctx** c) {
    *c = tdbp_plan_live(p) ? p->ctx : nullptr;
    if (!pointers_ok) return fail(*c, SARX_ERR_INVALID, "NULL pointer");
    if (!img128 && !img64) return fail(*c, SARX_ERR_INVALID, "both outputs are NULL");
    if (((uintptr_t)img128 & 15) || ((uintptr_t)img64 & 7)) return fail(*c, SARX_ERR_INVALID, "misaligned images128 (16) or images64 (8)");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(vel_focus[i])) return fail(*c, SARX_ERR_INVALID, "vel_focus has a non-finite component");
    if (const int rc = tdbp_scene_check(*c, scene_size)) return rc;
    if (const int rc = tdbp_multi_params_check(*c, -1, k)) return rc;
    for (int ch = 0; ch < k->n_rx; ++ch)
        if (!raw[ch]) return fail(*c, SARX_ERR_INVALID, "NULL pointer for the raw pulses of channel %d", ch);
    if (const int rc = tdbp_plan_usable(p, c)) return rc;
    if (const int rc = tdbp_multi_params_check(*c, p->n_p, k)) return rc;
    return tdbp_vel_tx_check(*c, vel_tx, p->n_p);
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
