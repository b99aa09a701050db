// libsarx C ABI of include/sarx_tdbp_pair_search.h: argument checks and the launches of tdbp_pair_search.hip.
#include "../../include/sarx_tdbp_pair_search.h"
#include "api_tdbp.h"
#include "tdbp_pair_search.h"

#include <string>
#include <vector>

using namespace sarx;

// what can be said of the search's parameter block; nx, ny < 1: the grid is not known yet, the chip is held to it later
static int params_check(sarx_ctx* c, const sarx_tdbp_pair_search_params* k, int nx, int ny) {
    if (!k) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (k->n_hyp < 1 || k->n_hyp > SARX_TDBP_PAIR_SEARCH_MAX_HYP)
        return fail(c, SARX_ERR_INVALID, "n_hyp %d must be 1 .. %d", k->n_hyp, SARX_TDBP_PAIR_SEARCH_MAX_HYP);
    if (k->chip_x < SARX_TDBP_PAIR_SEARCH_MIN_CHIP || k->chip_x > SARX_TDBP_PAIR_SEARCH_MAX_CHIP || k->chip_y < SARX_TDBP_PAIR_SEARCH_MIN_CHIP ||
        k->chip_y > SARX_TDBP_PAIR_SEARCH_MAX_CHIP)
        return fail(c, SARX_ERR_INVALID, "chip %d x %d: both sides must be %d .. %d", k->chip_y, k->chip_x, SARX_TDBP_PAIR_SEARCH_MIN_CHIP,
                    SARX_TDBP_PAIR_SEARCH_MAX_CHIP);
    if (k->source != SARX_TDBP_PAIR_SEARCH_DPCA && k->source != SARX_TDBP_PAIR_SEARCH_CH0)
        return fail(c, SARX_ERR_INVALID, "unknown source %d", k->source);
    if ((nx > 0 && k->chip_x > nx) || (ny > 0 && k->chip_y > ny))
        return fail(c, SARX_ERR_INVALID, "chip %d x %d is larger than the grid %d x %d", k->chip_y, k->chip_x, ny, nx);
    return SARX_OK;
}

// Everything that can be refused without reading the plan is refused first, so a caller without a device gets the same answers.
// The plan next; last what needs the plan: the upper end of the pulse ranges, the chip against the grid, the rows of vel_tx.
static int search_check(sarx_tdbp_plan* p, bool pointers_ok, const double* vel_tx, double scene_size, const sarx_tdbp_pair_params* pair,
                        const double* vel_hyps, const void* reports, const void* header, int max_det, const sarx_tdbp_pair_search_params* k,
                        const void* records, const void* best, const void* chips, sarx_ctx** c) {
    *c = tdbp_plan_live(p) ? p->ctx : nullptr;
    if (!pointers_ok) return fail(*c, SARX_ERR_INVALID, "NULL pointer");
    if (((uintptr_t)reports & 7) || ((uintptr_t)header & 3) || ((uintptr_t)records & 7) || ((uintptr_t)best & 7) || ((uintptr_t)chips & 15))
        return fail(*c, SARX_ERR_INVALID, "misaligned reports (8), header (4), records (8), best (8) or chips (16)");
    if (const int rc = params_check(*c, k, 0, 0)) return rc;
    if (max_det < 1) return fail(*c, SARX_ERR_INVALID, "max_detections %d must be >= 1", max_det);
    if ((long long)max_det * k->n_hyp > SARX_TDBP_PAIR_SEARCH_MAX_CHIPS)
        return fail(*c, SARX_ERR_INVALID, "max_detections %d x n_hyp %d = %lld chips, more than %d", max_det, k->n_hyp,
                    (long long)max_det * k->n_hyp, SARX_TDBP_PAIR_SEARCH_MAX_CHIPS);
    if (const int rc = tdbp_hyps_check(*c, vel_hyps, k->n_hyp)) return rc;
    if (const int rc = tdbp_scene_check(*c, scene_size)) return rc;
    if (const int rc = tdbp_pair_params_check(*c, -1, pair)) return rc;          // the pulse count is not known yet
    if (const int rc = tdbp_plan_usable(p, c)) return rc;
    if (const int rc = tdbp_pair_params_check(*c, p->n_p, pair)) return rc;
    if (const int rc = params_check(*c, k, p->nx, p->ny)) return rc;
    return tdbp_vel_tx_check(*c, vel_tx, p->n_p);
}

// the launches; a combination whose partial sums do not fit is the caller's mistake, not the device's
static int run(sarx_ctx* c, sarx_tdbp_plan* p, const float2* d_raw0, const float2* d_raw1, const double* pos_tx, const double* vel_tx,
               const double* t_pulses, double t_start, double scene_size, const sarx_tdbp_pair_params* pair, const double* vel_hyps,
               const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_det, const sarx_tdbp_pair_search_params* k,
               sarx_tdbp_search_record* d_records, sarx_tdbp_pair_search_best* d_best, void* d_chips) {
    std::string why;
    const hipError_t e = tdbp_pair_search(p->t, d_raw0, d_raw1, pos_tx, vel_tx, t_pulses, t_start, scene_size, pair, vel_hyps, d_reports, d_header,
                                          max_det, k, p->search_chunks, d_records, d_best, (double2*)d_chips, &why, c->stream);
    if (e == hipErrorInvalidValue && !why.empty()) return fail(c, SARX_ERR_INVALID, "%s", why.c_str());
    HIPCHK(c, e);
    return SARX_OK;
}

extern "C" {

int sarx_tdbp_pair_search_check(const sarx_tdbp_pair_search_params* params, int nx, int ny) {
    if (nx < 0 || ny < 0) return fail(nullptr, SARX_ERR_INVALID, "grid %d x %d must not be negative", ny, nx);
    return params_check(nullptr, params, nx, ny);
}

int sarx_tdbp_pair_search_dev(sarx_tdbp_plan* p, const void* d_raw0, const void* d_raw1, const double* pos_tx, const double* vel_tx,
                              const double* t_pulses, double t_start, double scene_size, const sarx_tdbp_pair_params* pair,
                              const double* vel_hyps, const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header,
                              int max_detections, const sarx_tdbp_pair_search_params* params, sarx_tdbp_search_record* d_records,
                              sarx_tdbp_pair_search_best* d_best, void* d_chips) {
    sarx_ctx* c = nullptr;
    const bool ptrs = d_raw0 && d_raw1 && pos_tx && vel_tx && t_pulses && pair && vel_hyps && d_reports && d_header && params && d_records && d_best;
    const int rc = search_check(p, ptrs, vel_tx, scene_size, pair, vel_hyps, d_reports, d_header, max_detections, params, d_records, d_best,
                                d_chips, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        return run(c, p, (const float2*)d_raw0, (const float2*)d_raw1, pos_tx, vel_tx, t_pulses, t_start, scene_size, pair, vel_hyps, d_reports,
                   d_header, max_detections, params, d_records, d_best, d_chips);
    });
}

int sarx_tdbp_pair_search_host(sarx_tdbp_plan* p, const void* raw0, const void* raw1, const double* pos_tx, const double* vel_tx,
                               const double* t_pulses, double t_start, double scene_size, const sarx_tdbp_pair_params* pair,
                               const double* vel_hyps, const sarx_gmti_report* reports, const sarx_gmti_header* header,
                               int max_detections, const sarx_tdbp_pair_search_params* params, sarx_tdbp_search_record* records,
                               sarx_tdbp_pair_search_best* best, void* chips) {
    sarx_ctx* c = nullptr;
    const bool ptrs = raw0 && raw1 && pos_tx && vel_tx && t_pulses && pair && vel_hyps && reports && header && params && records && best;
    const int rc = search_check(p, ptrs, vel_tx, scene_size, pair, vel_hyps, reports, header, max_detections, params, records, best, chips, &c);
    if (rc != SARX_OK) return rc;
    return guarded(c, [&] {
        const size_t n = (size_t)p->n_p * p->n_s, n_hyp = (size_t)params->n_hyp;
        const size_t chip_bytes = 2 * (size_t)params->chip_x * params->chip_y * sizeof(double2);      // both channels of one hypothesis
        if (const int rc = tdbp_plan_raw(c, p)) return rc;
        PairSearchStaging s{};
        HIPCHK(c, tdbp_pair_search_staging(p->t, max_detections, params, chips != nullptr, &s));
        // the slot as the device form reads it: the header, then as many reports as it counts and the list holds
        const bool usable = header->overflow == 0 && header->count <= (uint32_t)max_detections;
        const size_t count = usable ? header->count : 0;
        sarx_gmti_header* d_header = (sarx_gmti_header*)s.slot;
        sarx_gmti_report* d_reports = (sarx_gmti_report*)(d_header + 1);
        HIPCHK(c, staged_copy(c, p->d_raw, raw0, n * sizeof(float2), true));
        HIPCHK(c, staged_copy(c, s.raw1, raw1, n * sizeof(float2), true));
        HIPCHK(c, hipMemcpyAsync(d_header, header, sizeof(sarx_gmti_header), hipMemcpyHostToDevice, c->stream));
        if (count) HIPCHK(c, hipMemcpyAsync(d_reports, reports, count * sizeof(sarx_gmti_report), hipMemcpyHostToDevice, c->stream));
        if (const int rc = run(c, p, p->d_raw, s.raw1, pos_tx, vel_tx, t_pulses, t_start, scene_size, pair, vel_hyps, d_reports, d_header,
                               max_detections, params, s.rec, s.best, s.chips))
            return rc;
        // back: only what the device form writes - a report outside the grid gets its k_best alone
        std::vector<sarx_tdbp_search_record> h_rec(count * n_hyp);
        std::vector<sarx_tdbp_pair_search_best> h_best(count);
        if (count) {
            HIPCHK(c, hipMemcpyAsync(h_rec.data(), s.rec, h_rec.size() * sizeof(sarx_tdbp_search_record), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_best.data(), s.best, h_best.size() * sizeof(sarx_tdbp_pair_search_best), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t r = 0; r < count; ++r) {
            const bool inside = reports[r].i >= 0 && reports[r].i < p->ny && reports[r].j >= 0 && reports[r].j < p->nx;
            if (!inside) { best[r].k_best = -1; continue; }
            best[r] = h_best[r];
            for (size_t h = 0; h < n_hyp; ++h) records[r * n_hyp + h] = h_rec[r * n_hyp + h];
            if (chips)
                HIPCHK(c, staged_copy(c, (char*)chips + r * n_hyp * chip_bytes, (const char*)s.chips + r * n_hyp * chip_bytes, n_hyp * chip_bytes, false));
        }
        return (int)SARX_OK;
    });
}

int sarx_tdbp_pair_search_route(const sarx_tdbp_plan* p, int* tile) {
    return tdbp_route_query(p, tdbp_pair_search_route, "the plan has not run a pair search yet", tile);
}

}  // extern "C"
