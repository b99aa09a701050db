// libsarx C ABI of include/sarx_gmti.h and include/sarx_refocus.h: parameter checks and the launches of gmti.hip and refocus.hip.
#include "../../include/sarx_refocus.h"
#include "api_ctx.h"
#include "gmti.h"
#include "refocus.h"

#include <cmath>

using namespace sarx;

extern "C" {

// ---- GMTI detection (include/sarx_gmti.h, gmti.hip) ---------------------------------------------------------------------------
static int gmti_check_params(sarx_ctx* c, const sarx_gmti_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "GMTI params is NULL");
    if (p->guard_az < 0 || p->guard_rg < 0 || p->train_az < 0 || p->train_rg < 0)
        return fail(c, SARX_ERR_INVALID, "GMTI half-widths must be >= 0 (guard %d x %d, train %d x %d)", p->guard_az, p->guard_rg,
                    p->train_az, p->train_rg);
    if (p->guard_az + p->train_az > SARX_GMTI_MAX_HALF || p->guard_rg + p->train_rg > SARX_GMTI_MAX_HALF)
        return fail(c, SARX_ERR_UNSUPPORTED, "GMTI guard + train half-widths %d x %d exceed %d", p->guard_az + p->train_az,
                    p->guard_rg + p->train_rg, SARX_GMTI_MAX_HALF);
    if (p->train_az == 0 && p->train_rg == 0) return fail(c, SARX_ERR_INVALID, "GMTI training set is empty (train half-widths 0 x 0)");
    if (!(p->alpha > 0.0) || !std::isfinite(p->alpha)) return fail(c, SARX_ERR_INVALID, "GMTI alpha must be finite and > 0");
    if (p->min_train < 1) return fail(c, SARX_ERR_INVALID, "GMTI min_train must be >= 1");
    if (p->max_detections < 1) return fail(c, SARX_ERR_INVALID, "GMTI max_detections must be >= 1");
    return SARX_OK;
}

int sarx_gmti_slot_bytes(const sarx_gmti_params* p, size_t* out) {
    if (!out) return fail(nullptr, SARX_ERR_INVALID, "out_bytes is NULL");
    const int rc = gmti_check_params(nullptr, p);
    if (rc != SARX_OK) return rc;
    *out = gmti_slot_bytes(p->max_detections);
    return SARX_OK;
}

int sarx_gmti_cfar_dev(sarx_ctx* c, const float* d_mag, int n_az, int n_rg, const sarx_gmti_params* p, sarx_gmti_report* d_reports,
                       sarx_gmti_header* d_header) {
    NEED_CTX(c);
    const int rc = gmti_check_params(c, p);
    if (rc != SARX_OK) return rc;
    if (!d_mag || !d_reports || !d_header) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
    if (n_az < 1 || n_rg < 1) return fail(c, SARX_ERR_INVALID, "bad plane size %d x %d", n_az, n_rg);
    if (((uintptr_t)d_reports & 7) || ((uintptr_t)d_header & 3)) return fail(c, SARX_ERR_INVALID, "misaligned report list or header");
    GmtiCfarArgs a{};
    a.m = d_mag; a.n_az = n_az; a.n_rg = n_rg;
    a.ga = p->guard_az; a.gr = p->guard_rg; a.oa = p->guard_az + p->train_az; a.orr = p->guard_rg + p->train_rg;
    a.alpha = p->alpha; a.min_train = p->min_train; a.max_det = p->max_detections;
    a.rep = d_reports; a.hdr = d_header;
    HIPCHK(c, launch_gmti_cfar(a, c->stream));
    return SARX_OK;
}

int sarx_gmti_refine_dev(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, double cal_phase,
                         sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_det) {
    NEED_CTX(c);
    if (!d_slc1 || !d_slc2 || !d_reports || !d_header) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
    if (n_az < 1 || n_rg < 1) return fail(c, SARX_ERR_INVALID, "bad image size %d x %d", n_az, n_rg);
    if (max_det < 1) return fail(c, SARX_ERR_INVALID, "max_detections must be >= 1");
    if (!std::isfinite(cal_phase)) return fail(c, SARX_ERR_INVALID, "cal_phase is not finite");
    if (((uintptr_t)d_reports & 7) || ((uintptr_t)d_header & 3)) return fail(c, SARX_ERR_INVALID, "misaligned report list or header");
    const int L = c->cur_lane;
    if (c->gmti_copy_cap[L] < (size_t)max_det) {         // grows only; a frame loop allocates once per lane
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(c->gmti_copy[L]));
        c->gmti_copy[L] = nullptr;
        c->gmti_copy_cap[L] = 0;
        HIPCHK(c, hipMalloc((void**)&c->gmti_copy[L], (size_t)max_det * sizeof(sarx_gmti_report)));
        c->gmti_copy_cap[L] = (size_t)max_det;
    }
    HIPCHK(c, hipMemcpyAsync(c->gmti_copy[L], d_reports, (size_t)max_det * sizeof(sarx_gmti_report), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, launch_gmti_refine((const float2*)d_slc1, (const float2*)d_slc2, n_az, n_rg, cal_phase, c->gmti_copy[L], d_reports, d_header,
                                 max_det, c->stream));
    return SARX_OK;
}

// ---- GMTI refocus (include/sarx_refocus.h, refocus.hip) ------------------------------------------------------------------------
static int refocus_check(sarx_ctx* c, const sarx_refocus_params* p, int n_az, int n_rg) {
    if (!p) return fail(c, SARX_ERR_INVALID, "refocus params is NULL");
    const int L = p->chip_az, W = p->chip_rg;
    if (L != 64 && L != 128 && L != 256 && L != 512) return fail(c, SARX_ERR_UNSUPPORTED, "refocus chip length %d is not 64, 128, 256 or 512", L);
    if (W < 1 || W > SARX_REFOCUS_MAX_W || W % 2 == 0)
        return fail(c, SARX_ERR_INVALID, "refocus chip width %d must be odd and 1 .. %d", W, SARX_REFOCUS_MAX_W);
    if (n_az < 1 || n_rg < 1) return fail(c, SARX_ERR_INVALID, "bad image size %d x %d", n_az, n_rg);
    if (L > n_az) return fail(c, SARX_ERR_INVALID, "refocus chip length %d exceeds the %d azimuth rows", L, n_az);
    if (p->source != SARX_REFOCUS_DPCA && p->source != SARX_REFOCUS_SLC1) return fail(c, SARX_ERR_INVALID, "refocus source %d unknown", p->source);
    if (p->n_hyp < 1 || p->n_hyp > SARX_REFOCUS_MAX_HYP)
        return fail(c, SARX_ERR_INVALID, "refocus n_hyp %d must be 1 .. %d", p->n_hyp, SARX_REFOCUS_MAX_HYP);
    const double pos[] = {p->wavelength_m, p->platform_speed_mps, p->prf_hz};
    for (double x : pos)
        if (!(x > 0.0) || !std::isfinite(x)) return fail(c, SARX_ERR_INVALID, "refocus wavelength, speed and prf must be finite and > 0");
    if (!std::isfinite(p->r0_m) || !std::isfinite(p->dr_m) || !std::isfinite(p->cal_phase))
        return fail(c, SARX_ERR_INVALID, "refocus r0, dr and cal_phase must be finite");
    for (int k = 0; k < p->n_hyp; ++k)
        if (!(p->speed_mps[k] > 0.0) || !std::isfinite(p->speed_mps[k]))
            return fail(c, SARX_ERR_INVALID, "refocus hypothesis %d: speed %g must be finite and > 0", k, p->speed_mps[k]);
    return SARX_OK;
}

int sarx_refocus_check(const sarx_refocus_params* p, int n_az, int n_rg) { return refocus_check(nullptr, p, n_az, n_rg); }

static int sarx_refocus_dev_impl(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, const sarx_refocus_params* p,
                                 const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_det,
                                 sarx_refocus_record* d_records, float* d_curves, void* d_chips) {
    const int rc = refocus_check(c, p, n_az, n_rg);
    if (rc != SARX_OK) return rc;
    if (!d_slc1 || !d_reports || !d_header || !d_records) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
    if (p->source == SARX_REFOCUS_DPCA && !d_slc2) return fail(c, SARX_ERR_INVALID, "the DPCA source needs slc2");
    if (max_det < 1) return fail(c, SARX_ERR_INVALID, "max_detections must be >= 1");
    if (((uintptr_t)d_slc1 & 7) || (d_slc2 && ((uintptr_t)d_slc2 & 7)) || ((uintptr_t)d_reports & 7) || ((uintptr_t)d_header & 3) ||
        ((uintptr_t)d_records & 7) || ((uintptr_t)d_curves & 3) || ((uintptr_t)d_chips & 7))
        return fail(c, SARX_ERR_INVALID, "misaligned image, report list, header, record, curve or chip buffer");
    RefocusArgs a{};
    a.s1 = (const float2*)d_slc1;
    if (p->source == SARX_REFOCUS_DPCA) {
        a.s2 = (const float2*)d_slc2;
        a.w2 = make_float2((float)cos(p->cal_phase), (float)sin(p->cal_phase));
    } else {
        a.s2 = a.s1;                                     // same loads in both modes, weighted by zero
        a.w2 = make_float2(0.f, 0.f);
    }
    a.n_az = n_az; a.n_rg = n_rg; a.L = p->chip_az; a.W = p->chip_rg; a.n_hyp = p->n_hyp;
    a.lam = p->wavelength_m; a.vr = p->platform_speed_mps; a.prf = p->prf_hz; a.r0 = p->r0_m; a.dr = p->dr_m;
    a.rep = d_reports; a.hdr = d_header; a.max_det = max_det;
    a.rec = d_records; a.chips = (float2*)d_chips;
    for (int k = 0; k < p->n_hyp; ++k) a.vp[k] = p->speed_mps[k];
    a.curves = d_curves;
    if (!a.curves) {
        const int L = c->cur_lane;
        const size_t need = (size_t)max_det * p->n_hyp;
        if (c->refocus_curves_cap[L] < need) {            // grows only; a frame loop allocates once per lane
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipFree(c->refocus_curves[L]));
            c->refocus_curves[L] = nullptr;
            c->refocus_curves_cap[L] = 0;
            HIPCHK(c, hipMalloc((void**)&c->refocus_curves[L], need * sizeof(float)));
            c->refocus_curves_cap[L] = need;
        }
        a.curves = c->refocus_curves[L];
    }
    HIPCHK(c, launch_refocus(a, c->stream));
    return SARX_OK;
}

int sarx_refocus_dev(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, const sarx_refocus_params* p,
                     const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_det, sarx_refocus_record* d_records,
                     float* d_curves, void* d_chips) {
    NEED_CTX(c);
    return guarded(c, [&] {
        return sarx_refocus_dev_impl(c, d_slc1, d_slc2, n_az, n_rg, p, d_reports, d_header, max_det, d_records, d_curves, d_chips);
    });
}

}  // extern "C"
