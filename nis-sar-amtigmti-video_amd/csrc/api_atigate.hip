// libsarx C ABI of include/sarx_atigate.h: parameter checks and the two launches of atigate.hip.
#include "../../include/sarx_atigate.h"
#include "api_gmti.h"
#include "atigate.h"

#include <cmath>

using namespace sarx;

extern "C" {

static int atigate_check(sarx_ctx* c, const sarx_atigate_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "ATI gate params is NULL");
    if (p->guard_az < 0 || p->guard_rg < 0 || p->train_az < 0 || p->train_rg < 0)
        return fail(c, SARX_ERR_INVALID, "ATI gate guard and train half-widths must be >= 0");
    if (p->guard_az > SARX_GMTI_MAX_HALF || p->train_az > SARX_GMTI_MAX_HALF || p->guard_az + p->train_az > SARX_GMTI_MAX_HALF ||
        p->guard_rg > SARX_GMTI_MAX_HALF || p->train_rg > SARX_GMTI_MAX_HALF || p->guard_rg + p->train_rg > SARX_GMTI_MAX_HALF)
        return fail(c, SARX_ERR_INVALID, "ATI gate guard + train half-widths exceed %d", SARX_GMTI_MAX_HALF);
    if (p->train_az == 0 && p->train_rg == 0) return fail(c, SARX_ERR_INVALID, "the ATI gate's training set is empty");
    if (p->look_az < 0 || p->look_az > SARX_ATIGATE_MAX_LOOK || p->look_rg < 0 || p->look_rg > SARX_ATIGATE_MAX_LOOK)
        return fail(c, SARX_ERR_INVALID, "ATI gate looks (%d, %d) must lie in 0 .. %d", p->look_az, p->look_rg, SARX_ATIGATE_MAX_LOOK);
    if (p->look_az > p->guard_az || p->look_rg > p->guard_rg)
        return fail(c, SARX_ERR_INVALID, "the ATI gate's look box (%d, %d) must lie inside its guard box (%d, %d)", p->look_az, p->look_rg,
                    p->guard_az, p->guard_rg);
    if (!(std::isfinite(p->k_sigma) && p->k_sigma >= 0.0)) return fail(c, SARX_ERR_INVALID, "ATI gate k_sigma must be finite and >= 0");
    if (!(p->phase_min >= 0.0 && p->phase_min <= 3.14159265358979323846))
        return fail(c, SARX_ERR_INVALID, "ATI gate phase_min must lie in 0 .. pi");
    if (!(p->min_coh >= 0.0 && p->min_coh <= 1.0)) return fail(c, SARX_ERR_INVALID, "ATI gate min_coh must lie in 0 .. 1");
    if (p->min_train < 1) return fail(c, SARX_ERR_INVALID, "ATI gate min_train %d must be >= 1", p->min_train);
    if (p->max_detections < 1 || p->max_detections > SARX_ATIGATE_MAX_DETECTIONS)
        return fail(c, SARX_ERR_INVALID, "ATI gate max_detections %d must be 1 .. %d", p->max_detections, SARX_ATIGATE_MAX_DETECTIONS);
    if ((p->flags & ~SARX_ATIGATE_KEEP_UNTESTED) != 0 || p->reserved != 0)
        return fail(c, SARX_ERR_INVALID, "ATI gate flags 0x%x: only bit 0 (KEEP_UNTESTED) is defined, reserved must be 0", p->flags);
    return SARX_OK;
}

int sarx_atigate_check(const sarx_atigate_params* p) { return atigate_check(nullptr, p); }

static size_t stats_bytes(const sarx_atigate_params* p) { return (size_t)p->max_detections * sizeof(sarx_atigate_stat); }

int sarx_atigate_stats_bytes(const sarx_atigate_params* p, size_t* out) {
    return size_query(out, [&] { return atigate_check(nullptr, p); }, [&] { return stats_bytes(p); });
}

int sarx_atigate_step_dev(sarx_ctx* c, const sarx_atigate_params* p, const void* d_slc1, const void* d_slc2, int n_az, int n_rg,
                          const void* d_slot_in, void* d_slot_out, void* d_stats) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = atigate_check(c, p)) return rc;
        const DevBuf bufs[] = {need(d_slc1, 8), need(d_slc2, 8), need(d_slot_in, 8), need(d_slot_out, 8), opt(d_stats, 8)};
        if (const int rc = buffers_present(c, bufs)) return rc;
        if (const int rc = plane_size_check(c, "image", n_az, n_rg, SARX_ATIGATE_MAX_DIM)) return rc;
        if (const int rc = buffers_aligned(c, bufs, "misaligned image, slot or statistics (8-byte alignment)")) return rc;
        const size_t slot = gmti_slot_bytes(p->max_detections);
        const size_t img = (size_t)n_az * (size_t)n_rg * sizeof(float2);
        const Span in[] = {{d_slot_in, slot}, {d_slc1, img}, {d_slc2, img}}, out_slot[] = {{d_slot_out, slot}};
        const Span rest[] = {in[0], in[1], in[2], out_slot[0]}, stats[] = {{d_stats, stats_bytes(p)}};
        if (const int rc = check_spans(c, in, out_slot, "the ATI gate's output slot overlaps an input", nullptr)) return rc;
        if (const int rc = check_spans(c, rest, stats, "the ATI gate's statistics overlap an input or the output slot", nullptr)) return rc;
        LaneScratch& keep = c->lane_scratch(sarx_ctx::ATIGATE_KEEP);      // its full size at once: allocated once per lane
        if (const int rc = keep.grow(c, (size_t)SARX_ATIGATE_MAX_DETECTIONS * sizeof(int32_t))) return rc;
        AtiGateArgs a{};
        a.p = *p;
        a.a = (const float2*)d_slc1;
        a.b = (const float2*)d_slc2;
        a.n_az = n_az;
        a.n_rg = n_rg;
        a.in = (const char*)d_slot_in;
        a.out = (char*)d_slot_out;
        a.stats = (sarx_atigate_stat*)d_stats;
        a.keep = (int32_t*)keep.p;
        HIPCHK(c, launch_atigate(a, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
