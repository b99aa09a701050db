// libsarx C ABI of include/sarx_tdbp_pair.h: argument checks and the launches of tdbp_pair.hip.
#include "../../include/sarx_tdbp_pair.h"
#include "api_tdbp.h"
#include "tdbp_pair.h"

using namespace sarx;

// Everything that can be refused without reading the plan is refused first, so a caller without a device gets the same answers.
// The plan next: NULL, or not (or no longer) one that sarx_tdbp_plan_create returned.  Last what needs the plan's pulse count: the
// upper end of the pulse ranges and the rows of vel_tx.  *c: where the message goes.
static int pair_check(sarx_tdbp_plan* p, bool pointers_ok, const double* vel_tx, const double* vel_focus, double scene_size,
                      const sarx_tdbp_pair_params* k, const void* img128, const void* img64, sarx_ctx** c) {
    *c = tdbp_plan_live(p) ? p->ctx : nullptr;
    if (!pointers_ok) return fail(*c, SARX_ERR_INVALID, "NULL pointer");
    if (!img128 && !img64) return fail(*c, SARX_ERR_INVALID, "both outputs are NULL");
    if (((uintptr_t)img128 & 15) || ((uintptr_t)img64 & 7)) return fail(*c, SARX_ERR_INVALID, "misaligned images128 (16) or images64 (8)");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(vel_focus[i])) return fail(*c, SARX_ERR_INVALID, "vel_focus has a non-finite component");
    if (const int rc = tdbp_scene_check(*c, scene_size)) return rc;
    if (const int rc = tdbp_pair_params_check(*c, -1, k)) return rc;
    if (const int rc = tdbp_plan_usable(p, c)) return rc;
    if (const int rc = tdbp_pair_params_check(*c, p->n_p, k)) return rc;
    return tdbp_vel_tx_check(*c, vel_tx, p->n_p);
}

extern "C" {

int sarx_tdbp_pair_check(int n_pulses, const sarx_tdbp_pair_params* params) {
    if (n_pulses < 1) return fail(nullptr, SARX_ERR_INVALID, "n_pulses %d must be >= 1", n_pulses);
    return tdbp_pair_params_check(nullptr, n_pulses, params);
}

int sarx_tdbp_pair_dev(sarx_tdbp_plan* p, const void* d_raw0, const void* d_raw1, const double* pos_tx, const double* vel_tx,
                       const double* t_pulses, double t_start, const double* vel_focus, double scene_size,
                       const sarx_tdbp_pair_params* params, void* d_images128, void* d_images64) {
    sarx_ctx* c = nullptr;
    const int rc = pair_check(p, d_raw0 && d_raw1 && pos_tx && vel_tx && t_pulses && vel_focus && params, vel_tx, vel_focus, scene_size,
                              params, d_images128, d_images64, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        HIPCHK(c, tdbp_pair(p->t, (const float2*)d_raw0, (const float2*)d_raw1, pos_tx, vel_tx, t_pulses, t_start, vel_focus, scene_size,
                            params, p->search_chunks, (double2*)d_images128, (float2*)d_images64, c->stream));
        return (int)SARX_OK;
    });
}

int sarx_tdbp_pair_host(sarx_tdbp_plan* p, const void* raw0, const void* raw1, const double* pos_tx, const double* vel_tx,
                        const double* t_pulses, double t_start, const double* vel_focus, double scene_size,
                        const sarx_tdbp_pair_params* params, void* images128, void* images64) {
    sarx_ctx* c = nullptr;
    const int rc = pair_check(p, raw0 && raw1 && pos_tx && vel_tx && t_pulses && vel_focus && params, vel_tx, vel_focus, scene_size, params,
                              images128, images64, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        const size_t n = (size_t)p->n_p * p->n_s, n_pix = (size_t)p->nx * p->ny;
        if (const int rc = tdbp_plan_raw(c, p)) return rc;
        float2* d_raw1 = nullptr;
        double2* d_128 = nullptr;
        float2* d_64 = nullptr;
        HIPCHK(c, tdbp_pair_staging(p->t, &d_raw1, &d_128, &d_64));
        HIPCHK(c, staged_copy(c, p->d_raw, raw0, n * sizeof(float2), true));
        HIPCHK(c, staged_copy(c, d_raw1, raw1, n * sizeof(float2), true));
        HIPCHK(c, tdbp_pair(p->t, p->d_raw, d_raw1, pos_tx, vel_tx, t_pulses, t_start, vel_focus, scene_size, params, p->search_chunks,
                            images128 ? d_128 : nullptr, images64 ? d_64 : nullptr, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (images128) HIPCHK(c, staged_copy(c, images128, d_128, 2 * n_pix * sizeof(double2), false));
        if (images64) HIPCHK(c, staged_copy(c, images64, d_64, 2 * n_pix * sizeof(float2), false));
        return (int)SARX_OK;
    });
}

int sarx_tdbp_pair_route(const sarx_tdbp_plan* p, int* tile) {
    return tdbp_route_query(p, tdbp_pair_route, "the plan has not run a pair call yet", tile);
}

}  // extern "C"
