// libsarx C ABI of include/sarx_tdbp_pair.h: the argument checks of the receiver stack (api_tdbp.h) at two channels and the launches of
// tdbp_pair.hip.
#include "../../include/sarx_tdbp_pair.h"
#include "api_tdbp.h"
#include "tdbp_pair.h"

using namespace sarx;

// tdbp_rx_check (api_tdbp.h) on the pair as the stack sees it: two channels; params may still be NULL, which pointers_ok says
static int pair_call_check(sarx_tdbp_plan* p, bool pointers_ok, const void* raw0, const void* raw1, const double* vel_tx, const double* vel_focus,
                           double scene_size, const sarx_tdbp_pair_params* k, const void* img128, const void* img64, sarx_ctx** c) {
    const void* const raw[2] = {raw0, raw1};
    const sarx_tdbp_multi_params m = k ? tdbp_pair_as_multi(*k) : sarx_tdbp_multi_params{};
    return tdbp_rx_check(p, pointers_ok, raw, vel_tx, vel_focus, scene_size, &m, img128, img64, c);
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
    const int rc = pair_call_check(p, d_raw0 && d_raw1 && pos_tx && vel_tx && t_pulses && vel_focus && params, d_raw0, d_raw1, vel_tx, vel_focus,
                              scene_size, params, d_images128, d_images64, &c);
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
    const int rc = pair_call_check(p, raw0 && raw1 && pos_tx && vel_tx && t_pulses && vel_focus && params, raw0, raw1, vel_tx, vel_focus,
                              scene_size, params, images128, images64, &c);
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
