// libsarx C ABI of include/sarx_oscfar.h: parameter checks and the launch of oscfar.hip.
#include "../../include/sarx_oscfar.h"
#include "api_gmti.h"
#include "oscfar.h"

using namespace sarx;

extern "C" {

static int oscfar_n_full(const sarx_gmti_params& b) {
    return (2 * (b.guard_az + b.train_az) + 1) * (2 * (b.guard_rg + b.train_rg) + 1) - (2 * b.guard_az + 1) * (2 * b.guard_rg + 1);
}

static int oscfar_check(sarx_ctx* c, const sarx_oscfar_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "OS-CFAR params is NULL");
    if (const int rc = gmti_check_params(c, &p->base)) return rc;        // the CA launch's own refusals, word for word
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
        if (const int rc = oscfar_check(c, p)) return rc;
        const DevBuf bufs[] = {need(d_mag, 4), need(d_reports, 8), need(d_header, 4)};
        if (const int rc = buffers_present(c, bufs)) return rc;
        if (const int rc = plane_size_check(c, "plane", n_az, n_rg)) return rc;
        if (const int rc = buffers_aligned(c, bufs, "misaligned plane, report list or header")) return rc;
        OsCfarArgs a{};
        a.base = gmti_cfar_args(d_mag, n_az, n_rg, p->base, d_reports, d_header);
        a.rank = p->rank; a.n_full = oscfar_n_full(p->base);
        HIPCHK(c, launch_gmti_oscfar(a, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
