// libsarx C ABI of include/sarx_gmti.h and include/sarx_refocus.h: parameter checks and the launches of gmti.hip and refocus.hip.
#include "../../include/sarx_refocus.h"
#include "api_gmti.h"
#include "refocus.h"

using namespace sarx;

extern "C" {

// ---- GMTI detection (include/sarx_gmti.h, gmti.hip) ---------------------------------------------------------------------------
int sarx_gmti_slot_bytes(const sarx_gmti_params* p, size_t* out) {
    return size_query(out, [&] { return gmti_check_params(nullptr, p); }, [&] { return gmti_slot_bytes(p->max_detections); });
}

int sarx_gmti_cfar_dev(sarx_ctx* c, const float* d_mag, int n_az, int n_rg, const sarx_gmti_params* p, sarx_gmti_report* d_reports,
                       sarx_gmti_header* d_header) {
    NEED_CTX(c);
    if (const int rc = gmti_check_params(c, p)) return rc;
    const DevBuf bufs[] = {need(d_mag, 1), need(d_reports, 8), need(d_header, 4)};      // the plane's alignment: not checked here
    if (const int rc = buffers_present(c, bufs)) return rc;
    if (const int rc = plane_size_check(c, "plane", n_az, n_rg)) return rc;
    if (const int rc = buffers_aligned(c, bufs, "misaligned report list or header")) return rc;
    HIPCHK(c, launch_gmti_cfar(gmti_cfar_args(d_mag, n_az, n_rg, *p, d_reports, d_header), c->stream));
    return SARX_OK;
}

int sarx_gmti_refine_dev(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, double cal_phase,
                         sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_det) {
    NEED_CTX(c);
    const DevBuf bufs[] = {need(d_slc1, 1), need(d_slc2, 1), need(d_reports, 8), need(d_header, 4)};
    if (const int rc = buffers_present(c, bufs)) return rc;
    if (const int rc = plane_size_check(c, "image", n_az, n_rg)) return rc;
    if (max_det < 1) return fail(c, SARX_ERR_INVALID, "max_detections must be >= 1");
    if (!std::isfinite(cal_phase)) return fail(c, SARX_ERR_INVALID, "cal_phase is not finite");
    if (const int rc = buffers_aligned(c, bufs, "misaligned report list or header")) return rc;
    const size_t list = (size_t)max_det * sizeof(sarx_gmti_report);
    LaneScratch& copy = c->lane_scratch(sarx_ctx::GMTI_COPY);
    if (const int rc = copy.grow(c, list)) return rc;
    HIPCHK(c, hipMemcpyAsync(copy.p, d_reports, list, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, launch_gmti_refine((const float2*)d_slc1, (const float2*)d_slc2, n_az, n_rg, cal_phase, (const sarx_gmti_report*)copy.p, d_reports,
                                 d_header, max_det, c->stream));
    return SARX_OK;
}

// ---- GMTI refocus (include/sarx_refocus.h, refocus.hip) ------------------------------------------------------------------------
static int refocus_check(sarx_ctx* c, const sarx_refocus_params* p, int n_az, int n_rg) {
    if (!p) return fail(c, SARX_ERR_INVALID, "refocus params is NULL");
    const int L = p->chip_az, W = p->chip_rg;
    if (L != 64 && L != 128 && L != 256 && L != 512) return fail(c, SARX_ERR_UNSUPPORTED, "refocus chip length %d is not 64, 128, 256 or 512", L);
    if (W < 1 || W > SARX_REFOCUS_MAX_W || W % 2 == 0)
        return fail(c, SARX_ERR_INVALID, "refocus chip width %d must be odd and 1 .. %d", W, SARX_REFOCUS_MAX_W);
    if (const int rc = plane_size_check(c, "image", n_az, n_rg)) return rc;
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
    if (const int rc = refocus_check(c, p, n_az, n_rg)) return rc;
    const DevBuf bufs[] = {need(d_slc1, 8), opt(d_slc2, 8), need(d_reports, 8), need(d_header, 4), need(d_records, 8), opt(d_curves, 4), opt(d_chips, 8)};
    if (const int rc = buffers_present(c, bufs)) return rc;
    if (p->source == SARX_REFOCUS_DPCA && !d_slc2) return fail(c, SARX_ERR_INVALID, "the DPCA source needs slc2");
    if (max_det < 1) return fail(c, SARX_ERR_INVALID, "max_detections must be >= 1");
    if (const int rc = buffers_aligned(c, bufs, "misaligned image, report list, header, record, curve or chip buffer")) return rc;
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
        LaneScratch& curves = c->lane_scratch(sarx_ctx::REFOCUS_CURVES);
        if (const int rc = curves.grow(c, (size_t)max_det * p->n_hyp * sizeof(float))) return rc;
        a.curves = (float*)curves.p;
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
