// libsarx C ABI of include/sarx_tdbp_search.h: argument checks and the launches of tdbp_search.hip.
#include "../../include/sarx_tdbp_search.h"
#include "api_tdbp.h"
#include "tdbp_search.h"

using namespace sarx;

extern "C" {

// Everything that can be refused without reading the plan is refused first, so a caller without a device gets the same answers.
// The plan last (tdbp_plan_usable).  *c: where the message goes.
static int search_check(sarx_tdbp_plan* p, bool pointers_ok, const double* vel_hyps, int n_hyp, const double* scene_size, sarx_ctx** c) {
    *c = tdbp_plan_live(p) ? p->ctx : nullptr;
    if (!pointers_ok) return fail(*c, SARX_ERR_INVALID, "NULL pointer");
    if (n_hyp < 1 || n_hyp > SARX_TDBP_SEARCH_MAX_HYP)
        return fail(*c, SARX_ERR_INVALID, "n_hyp %d must be 1 .. %d", n_hyp, SARX_TDBP_SEARCH_MAX_HYP);
    if (vel_hyps)
        if (const int rc = tdbp_hyps_check(*c, vel_hyps, n_hyp)) return rc;
    if (scene_size)
        if (const int rc = tdbp_scene_check(*c, *scene_size)) return rc;
    return tdbp_plan_usable(p, c);
}

int sarx_tdbp_search_dev(sarx_tdbp_plan* p, const void* d_raw, const double* pos, const double* vel, const double* t_pulses,
                         double t_start, const double* vel_hyps, int n_hyp, double scene_size, void* d_images,
                         sarx_tdbp_search_record* d_records) {
    sarx_ctx* c = nullptr;
    const int rc = search_check(p, d_raw && pos && vel && t_pulses && vel_hyps && d_records, vel_hyps, n_hyp, &scene_size, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        if (((uintptr_t)d_records & 7) || ((uintptr_t)d_images & 15)) return fail(c, SARX_ERR_INVALID, "misaligned records (8) or images (16)");
        HIPCHK(c, tdbp_search(p->t, (const float2*)d_raw, pos, vel, t_pulses, t_start, vel_hyps, n_hyp, scene_size, p->search_chunks,
                              (double2*)d_images, d_records, c->stream));
        return (int)SARX_OK;
    });
}

int sarx_tdbp_search_host(sarx_tdbp_plan* p, const void* raw, const double* pos, const double* vel, const double* t_pulses,
                          double t_start, const double* vel_hyps, int n_hyp, double scene_size, void* images,
                          sarx_tdbp_search_record* records) {
    sarx_ctx* c = nullptr;
    const int rc = search_check(p, raw && pos && vel && t_pulses && vel_hyps && records, vel_hyps, n_hyp, &scene_size, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        const size_t n = (size_t)p->n_p * p->n_s, n_pix = (size_t)p->nx * p->ny;
        if (const int rc = tdbp_plan_raw(c, p)) return rc;
        HIPCHK(c, staged_copy(c, p->d_raw, raw, n * sizeof(float2), true));
        sarx_tdbp_search_record* d_rec = nullptr;
        double2* d_img = nullptr;
        HIPCHK(c, tdbp_search_staging(p->t, n_hyp, images != nullptr, &d_rec, &d_img, c->stream));
        HIPCHK(c, tdbp_search(p->t, p->d_raw, pos, vel, t_pulses, t_start, vel_hyps, n_hyp, scene_size, p->search_chunks, d_img, d_rec,
                              c->stream));
        HIPCHK(c, hipMemcpyAsync(records, d_rec, (size_t)n_hyp * sizeof(sarx_tdbp_search_record), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (images) HIPCHK(c, staged_copy(c, images, d_img, (size_t)n_hyp * n_pix * sizeof(double2), false));
        return (int)SARX_OK;
    });
}

int sarx_tdbp_search_route(const sarx_tdbp_plan* p, int* tile) {
    return tdbp_route_query(p, tdbp_search_route, "the plan has not run a search yet", tile);
}

int sarx_tdbp_search_set_chunks(sarx_tdbp_plan* p, int chunks) {
    if (chunks < 0 || chunks > SARX_TDBP_SEARCH_MAX_CHUNKS)
        return fail(tdbp_plan_live(p) ? p->ctx : nullptr, SARX_ERR_INVALID, "chunks %d must be 0 .. %d", chunks, SARX_TDBP_SEARCH_MAX_CHUNKS);
    sarx_ctx* c = nullptr;
    if (const int rc = tdbp_plan_usable(p, &c)) return rc;
    p->search_chunks = chunks;
    return SARX_OK;
}

int sarx_tdbp_search_metric_dev(sarx_tdbp_plan* p, const void* d_stack, int n_hyp, sarx_tdbp_search_record* d_records) {
    sarx_ctx* c = nullptr;
    const int rc = search_check(p, d_stack && d_records, nullptr, n_hyp, nullptr, &c);
    if (rc != SARX_OK) return rc;
    if (((uintptr_t)d_records & 7) || ((uintptr_t)d_stack & 15)) return fail(c, SARX_ERR_INVALID, "misaligned records (8) or stack (16)");
    HIPCHK(c, tdbp_search_metric(p->t, (const double2*)d_stack, n_hyp, d_records, c->stream));
    return SARX_OK;
}

}  // extern "C"
