// libsarx C ABI of include/sarx_oscfar.h: parameter checks and the launch of oscfar.hip.
#include "../../include/sarx_oscfar.h"
#include "api_ctx.h"
#include "oscfar.h"

using namespace sarx;

extern "C" {

static int oscfar_n_full(const sarx_gmti_params& b) {
    return (2 * (b.guard_az + b.train_az) + 1) * (2 * (b.guard_rg + b.train_rg) + 1) - (2 * b.guard_az + 1) * (2 * b.guard_rg + 1);
}

static int oscfar_check(sarx_ctx* c, const sarx_oscfar_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "OS-CFAR params is NULL");
    size_t bytes = 0;
    const int rc = sarx_gmti_slot_bytes(&p->base, &bytes);        // the CA launch's own refusals, word for word
    if (rc != SARX_OK) return c ? fail(c, rc, "%s", sarx_last_error(nullptr)) : rc;
    if (p->flags != 0) return fail(c, SARX_ERR_INVALID, "OS-CFAR flags %d: none is defined", p->flags);
    const int nf = oscfar_n_full(p->base);
    if (p->rank < 1 || p->rank > nf) return fail(c, SARX_ERR_INVALID, "OS-CFAR rank %d must be 1 .. N_full = %d", p->rank, nf);
    return SARX_OK;
}

int sarx_oscfar_check(const sarx_oscfar_params* p) { return oscfar_check(nullptr, p); }

int sarx_gmti_oscfar_dev(sarx_ctx* c, const float* d_mag, int n_az, int n_rg, const sarx_oscfar_params* p, sarx_gmti_report* d_reports,
                         sarx_gmti_header* d_header) {
    NEED_CTX(c);
    return guarded(c, [&] {
        const int rc = oscfar_check(c, p);
        if (rc != SARX_OK) return rc;
        if (!d_mag || !d_reports || !d_header) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
        if (n_az < 1 || n_rg < 1) return fail(c, SARX_ERR_INVALID, "bad plane size %d x %d", n_az, n_rg);
        if (((uintptr_t)d_mag & 3) || ((uintptr_t)d_reports & 7) || ((uintptr_t)d_header & 3))
            return fail(c, SARX_ERR_INVALID, "misaligned plane, report list or header");
        OsCfarArgs a{};
        const sarx_gmti_params& b = p->base;
        a.base.m = d_mag; a.base.n_az = n_az; a.base.n_rg = n_rg;
        a.base.ga = b.guard_az; a.base.gr = b.guard_rg; a.base.oa = b.guard_az + b.train_az; a.base.orr = b.guard_rg + b.train_rg;
        a.base.alpha = b.alpha; a.base.min_train = b.min_train; a.base.max_det = b.max_detections;
        a.base.rep = d_reports; a.base.hdr = d_header;
        a.rank = p->rank; a.n_full = oscfar_n_full(b);
        HIPCHK(c, launch_gmti_oscfar(a, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
