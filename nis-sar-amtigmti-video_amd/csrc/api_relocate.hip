// libsarx C ABI of include/sarx_relocate.h: parameter checks and the two launches of relocate.hip.
#include "../../include/sarx_relocate.h"
#include "api_gmti.h"
#include "relocate.h"

using namespace sarx;

static int relocate_check(sarx_ctx* c, const sarx_relocate_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "relocation params is NULL");
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(p->pos_ref[k])) return fail(c, SARX_ERR_INVALID, "pos_ref[%d] must be finite", k);
        if (!std::isfinite(p->vel_ref[k])) return fail(c, SARX_ERR_INVALID, "vel_ref[%d] must be finite", k);
    }
    const struct { const char* name; double v; bool step; } f[] = {
        {"in_x0", p->in_x0, false},   {"in_y0", p->in_y0, false},   {"in_dx", p->in_dx, true},   {"in_dy", p->in_dy, true},
        {"out_x0", p->out_x0, false}, {"out_y0", p->out_y0, false}, {"out_dx", p->out_dx, true}, {"out_dy", p->out_dy, true}};
    for (const auto& x : f) {
        if (!std::isfinite(x.v)) return fail(c, SARX_ERR_INVALID, "%s must be finite", x.name);
        if (x.step && x.v == 0.0) return fail(c, SARX_ERR_INVALID, "%s must not be 0", x.name);
    }
    if (p->out_nx < 1 || p->out_nx > SARX_TDBP_MULTI_MAX_DIM) return fail(c, SARX_ERR_INVALID, "out_nx %d must be 1 .. %d", p->out_nx, SARX_TDBP_MULTI_MAX_DIM);
    if (p->out_ny < 1 || p->out_ny > SARX_TDBP_MULTI_MAX_DIM) return fail(c, SARX_ERR_INVALID, "out_ny %d must be 1 .. %d", p->out_ny, SARX_TDBP_MULTI_MAX_DIM);
    if (p->max_detections < 1 || p->max_detections > SARX_TDBP_MULTI_MAX_DETECTIONS)
        return fail(c, SARX_ERR_INVALID, "max_detections %d must be 1 .. %d", p->max_detections, SARX_TDBP_MULTI_MAX_DETECTIONS);
    if (p->reserved != 0) return fail(c, SARX_ERR_INVALID, "reserved must be 0");
    return SARX_OK;
}

// a per-report input array: n elements of `elem` bytes, `stride` bytes apart
static bool array_stride_ok(size_t stride, size_t elem) { return stride >= elem && stride % elem == 0; }
static Span array_span(const void* p, size_t stride, size_t elem, size_t n) { return {p, (n - 1) * stride + elem}; }

extern "C" {

int sarx_relocate_check(const sarx_relocate_params* params) { return relocate_check(nullptr, params); }

int sarx_relocate_dev(sarx_ctx* c, const sarx_relocate_params* p, const void* d_slot, const void* d_v_los, size_t v_los_stride,
                      const void* d_valid, size_t valid_stride, const void* d_v_along, size_t v_along_stride, void* d_records,
                      void* d_out_slot) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = relocate_check(c, p)) return rc;
        const DevBuf bufs[] = {need(d_slot, 8), need(d_v_los, 8), opt(d_valid, 4), opt(d_v_along, 8), need(d_records, 8), need(d_out_slot, 8)};
        if (const int rc = buffers_present(c, bufs)) return rc;
        if (!array_stride_ok(v_los_stride, 8)) return fail(c, SARX_ERR_INVALID, "v_los_stride %zu must be a multiple of 8, >= 8", v_los_stride);
        if (d_valid && !array_stride_ok(valid_stride, 4)) return fail(c, SARX_ERR_INVALID, "valid_stride %zu must be a multiple of 4, >= 4", valid_stride);
        if (d_v_along && !array_stride_ok(v_along_stride, 8))
            return fail(c, SARX_ERR_INVALID, "v_along_stride %zu must be a multiple of 8, >= 8", v_along_stride);
        if (const int rc = buffers_aligned(c, bufs, "misaligned slot, speeds, records (8-byte alignment) or valid words (4-byte)")) return rc;
        const size_t md = (size_t)p->max_detections, slot = gmti_slot_bytes(p->max_detections);
        const Span in[] = {{d_slot, slot}, array_span(d_v_los, v_los_stride, 8, md), array_span(d_valid, valid_stride, 4, md),
                           array_span(d_v_along, v_along_stride, 8, md)};
        const Span out[] = {{d_records, md * sizeof(sarx_relocate_record)}, {d_out_slot, slot}};
        if (const int rc = check_spans(c, in, out, "the relocation's records or output slot overlap an input",
                                       "the relocation's records overlap its output slot"))
            return rc;
        LaneScratch& keys = c->lane_scratch(sarx_ctx::RELOCATE_KEYS);      // its full size at once: allocated once per lane
        if (const int rc = keys.grow(c, (size_t)SARX_TDBP_MULTI_MAX_DETECTIONS * sizeof(long long))) return rc;
        RelocateArgs a{};
        a.p = *p;
        a.in = (const char*)d_slot;
        a.v_los = (const char*)d_v_los;
        a.valid = (const char*)d_valid;
        a.v_along = (const char*)d_v_along;
        a.v_los_stride = v_los_stride;
        a.valid_stride = valid_stride;
        a.v_along_stride = v_along_stride;
        a.rec = (sarx_relocate_record*)d_records;
        a.out = (char*)d_out_slot;
        a.keys = (long long*)keys.p;
        HIPCHK(c, launch_relocate(a, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
