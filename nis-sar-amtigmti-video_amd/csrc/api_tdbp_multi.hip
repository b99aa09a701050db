// libsarx C ABI of include/sarx_tdbp_multi.h: argument checks and the launches of tdbp_multi.hip.
#include "../../include/sarx_tdbp_multi.h"
#include "api_gmti.h"
#include "api_tdbp.h"
#include "tdbp_multi.h"

using namespace sarx;

static int resolve_check(sarx_ctx* c, const sarx_tdbp_multi_resolve_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "resolver params is NULL");
    if (p->n_rx < 2 || p->n_rx > SARX_TDBP_MULTI_MAX_RX) return fail(c, SARX_ERR_INVALID, "n_rx %d must be 2 .. %d", p->n_rx, SARX_TDBP_MULTI_MAX_RX);
    double longest = 0.0;
    for (int b = 0; b < 3; ++b) {
        if (b < p->n_rx - 1) {
            if (!std::isfinite(p->lag_s[b]) || p->lag_s[b] == 0.0) return fail(c, SARX_ERR_INVALID, "lag_s[%d] must be finite and non-zero", b);
            longest = std::fmax(longest, std::fabs(p->lag_s[b]));
        } else if (!(p->lag_s[b] == 0.0)) {
            return fail(c, SARX_ERR_INVALID, "unused slot %d of lag_s must be 0", b);
        }
    }
    if (!(p->wavelength_m > 0.0) || !std::isfinite(p->wavelength_m)) return fail(c, SARX_ERR_INVALID, "wavelength_m must be finite and > 0");
    if (!(p->v_max_mps > 0.0) || !std::isfinite(p->v_max_mps)) return fail(c, SARX_ERR_INVALID, "v_max_mps must be finite and > 0");
    if (p->half < 0 || p->half > SARX_TDBP_MULTI_MAX_HALF) return fail(c, SARX_ERR_INVALID, "half %d must be 0 .. %d", p->half, SARX_TDBP_MULTI_MAX_HALF);
    if (p->max_detections < 1 || p->max_detections > SARX_TDBP_MULTI_MAX_DETECTIONS)
        return fail(c, SARX_ERR_INVALID, "max_detections %d must be 1 .. %d", p->max_detections, SARX_TDBP_MULTI_MAX_DETECTIONS);
    if (p->reserved != 0) return fail(c, SARX_ERR_INVALID, "reserved must be 0");
    // the candidates are the integers of an interval 4 |lag_B| v_max / lambda long: at most its floor + 1 of them
    const double span = 4.0 * longest * p->v_max_mps / p->wavelength_m;
    if (!(std::floor(span) + 1.0 <= (double)SARX_TDBP_MULTI_MAX_CANDIDATES))
        return fail(c, SARX_ERR_INVALID, "v_max_mps allows too many candidates: %.0f wraps of the longest baseline, at most %d", std::floor(span) + 1.0,
                    SARX_TDBP_MULTI_MAX_CANDIDATES);
    return SARX_OK;
}

extern "C" {

int sarx_tdbp_multi_check(int n_pulses, const sarx_tdbp_multi_params* params) {
    if (n_pulses < 1) return fail(nullptr, SARX_ERR_INVALID, "n_pulses %d must be >= 1", n_pulses);
    return tdbp_multi_params_check(nullptr, n_pulses, params);
}

int sarx_tdbp_multi_dev(sarx_tdbp_plan* p, const void* const* d_raw, const double* pos_tx, const double* vel_tx, const double* t_pulses,
                        double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* params,
                        void* d_images128, void* d_images64) {
    sarx_ctx* c = nullptr;
    const int rc = tdbp_rx_check(p, d_raw && pos_tx && vel_tx && t_pulses && vel_focus && params, d_raw, vel_tx, vel_focus, scene_size, params,
                               d_images128, d_images64, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        HIPCHK(c, tdbp_multi(p->t, (const float2* const*)d_raw, pos_tx, vel_tx, t_pulses, t_start, vel_focus, scene_size, params,
                             p->search_chunks, (double2*)d_images128, (float2*)d_images64, c->stream));
        return (int)SARX_OK;
    });
}

int sarx_tdbp_multi_host(sarx_tdbp_plan* p, const void* const* raw, const double* pos_tx, const double* vel_tx, const double* t_pulses,
                         double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* params,
                         void* images128, void* images64) {
    sarx_ctx* c = nullptr;
    const int rc = tdbp_rx_check(p, raw && pos_tx && vel_tx && t_pulses && vel_focus && params, raw, vel_tx, vel_focus, scene_size, params,
                               images128, images64, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        const size_t n = (size_t)p->n_p * p->n_s, n_pix = (size_t)p->nx * p->ny;
        const int n_rx = params->n_rx;
        if (const int rc = tdbp_plan_raw(c, p)) return rc;
        float2* d_raw[SARX_TDBP_MULTI_MAX_RX] = {p->d_raw, nullptr, nullptr, nullptr};
        double2* d_128 = nullptr;
        float2* d_64 = nullptr;
        HIPCHK(c, tdbp_multi_staging(p->t, n_rx, d_raw + 1, &d_128, &d_64));
        for (int ch = 0; ch < n_rx; ++ch) HIPCHK(c, staged_copy(c, d_raw[ch], raw[ch], n * sizeof(float2), true));
        HIPCHK(c, tdbp_multi(p->t, d_raw, pos_tx, vel_tx, t_pulses, t_start, vel_focus, scene_size, params, p->search_chunks,
                             images128 ? d_128 : nullptr, images64 ? d_64 : nullptr, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (images128) HIPCHK(c, staged_copy(c, images128, d_128, n_rx * n_pix * sizeof(double2), false));
        if (images64) HIPCHK(c, staged_copy(c, images64, d_64, n_rx * n_pix * sizeof(float2), false));
        return (int)SARX_OK;
    });
}

int sarx_tdbp_multi_route(const sarx_tdbp_plan* p, int* tile) {
    return tdbp_route_query(p, tdbp_multi_route, "the plan has not run a multi call yet", tile);
}

int sarx_tdbp_multi_scratch(const sarx_tdbp_plan* p, uint64_t* bytes, uint64_t* id) {
    if (!bytes || !id) return fail(nullptr, SARX_ERR_INVALID, "NULL pointer");
    sarx_ctx* c = nullptr;
    if (const int rc = tdbp_plan_usable(p, &c)) return rc;
    tdbp_multi_held(p->t, bytes, id);
    return SARX_OK;
}

int sarx_tdbp_multi_resolve_check(const sarx_tdbp_multi_resolve_params* params) { return resolve_check(nullptr, params); }

int sarx_tdbp_multi_resolve_dev(sarx_ctx* c, const sarx_tdbp_multi_resolve_params* p, const void* d_images64, int ny, int nx,
                                const void* d_slot, void* d_records) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = resolve_check(c, p)) return rc;
        const DevBuf bufs[] = {need(d_images64, 8), need(d_slot, 8), need(d_records, 8)};
        if (const int rc = buffers_present(c, bufs)) return rc;
        if (const int rc = plane_size_check(c, "image", ny, nx, SARX_TDBP_MULTI_MAX_DIM)) return rc;
        if (const int rc = buffers_aligned(c, bufs, "misaligned images, slot or records (8-byte alignment)")) return rc;
        const Span in[] = {{d_images64, (size_t)p->n_rx * (size_t)ny * (size_t)nx * sizeof(float2)}, {d_slot, gmti_slot_bytes(p->max_detections)}};
        const Span out[] = {{d_records, (size_t)p->max_detections * sizeof(sarx_tdbp_multi_record)}};
        if (const int rc = check_spans(c, in, out, "the resolver's records overlap an input", nullptr)) return rc;
        MultiResolveArgs a{};
        a.p = *p;
        a.imgs = (const float2*)d_images64;
        a.slot = (const char*)d_slot;
        a.rec = (sarx_tdbp_multi_record*)d_records;
        a.ny = ny;
        a.nx = nx;
        HIPCHK(c, launch_multi_resolve(a, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
