// The argument rules that the host units of the detection chain have in common (api_gmti.hip, api_oscfar.hip, api_cluster.hip,
// api_atigate.hip, api_track.hip, api_balance.hip, api_coherence.hip), each stated once: size queries, device buffers, image sizes,
// slots and tables, overlap, the CA-CFAR's parameter block.  Every helper refuses through fail(c, ...) and returns its code; the
// caller passes the words that are its own.  Host only: no kernel file includes this header.
#pragma once
#include "api_ctx.h"
#include "gmti.h"

#include <cmath>

namespace sarx {

// a *_bytes query: check() speaks for the parameters, size() is evaluated only once they are good
template <class Check, class Size> int size_query(size_t* out, Check check, Size size) {
    if (!out) return fail(nullptr, SARX_ERR_INVALID, "out_bytes is NULL");
    if (const int rc = check()) return rc;
    *out = size();
    return SARX_OK;
}

// ---- device buffers: an entry point declares them once, in the order its message names them -------------------------------------------
struct DevBuf { const void* p; unsigned align; bool required; };     // align: 4 or 8 bytes (1: not checked here); not required: may be NULL
inline DevBuf need(const void* p, unsigned align) { return {p, align, true}; }
inline DevBuf opt(const void* p, unsigned align) { return {p, align, false}; }
template <size_t N> int buffers_present(sarx_ctx* c, const DevBuf (&b)[N]) {
    for (const DevBuf& x : b)
        if (x.required && !x.p) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
    return SARX_OK;
}
template <size_t N> int buffers_aligned(sarx_ctx* c, const DevBuf (&b)[N], const char* misaligned) {
    for (const DevBuf& x : b)
        if ((uintptr_t)x.p & (x.align - 1)) return fail(c, SARX_ERR_INVALID, "%s", misaligned);
    return SARX_OK;
}
// a missing required buffer first, a misaligned one second; an entry point with refusals of its own between the two calls the halves
template <size_t N> int buffers_ok(sarx_ctx* c, const DevBuf (&b)[N], const char* misaligned) {
    if (const int rc = buffers_present(c, b)) return rc;
    return buffers_aligned(c, b, misaligned);
}

// an image ("image") or a magnitude plane ("plane") of n_az x n_rg; max_dim > 0 bounds each side: in who's name as SARX_ERR_UNSUPPORTED,
// without one as the same SARX_ERR_INVALID
inline int plane_size_check(sarx_ctx* c, const char* what, int n_az, int n_rg, int max_dim = 0, const char* who = nullptr) {
    const bool over = max_dim > 0 && (n_az > max_dim || n_rg > max_dim);
    if (n_az < 1 || n_rg < 1 || (over && !who)) return fail(c, SARX_ERR_INVALID, "bad %s size %d x %d", what, n_az, n_rg);
    if (over) return fail(c, SARX_ERR_UNSUPPORTED, "%s image size %d x %d exceeds %d per side", who, n_az, n_rg, max_dim);
    return SARX_OK;
}

// ---- slots and tables: a header, then its records (include/sarx_gmti.h, sarx_track.h, sarx_balance.h) -------------------------------
template <class H, class R> size_t table_bytes(size_t n) { return sizeof(H) + n * sizeof(R); }
inline size_t gmti_slot_bytes(int max_detections) { return table_bytes<sarx_gmti_header, sarx_gmti_report>((size_t)max_detections); }
// the records behind the header at p: R = [const] sarx_gmti_report, sarx_track_slot, sarx_balance_record
template <class H, class R> R* records_of(const void* p) { return (R*)((const char*)p + sizeof(H)); }
inline const sarx_gmti_report* slot_reports(const void* slot) { return records_of<sarx_gmti_header, const sarx_gmti_report>(slot); }
// the stride between the slots, plot records or images of consecutive frames: a multiple of 8 and at least one frame's bytes
inline bool stride_ok(size_t stride, size_t bytes) { return stride >= bytes && !(stride & 7); }

// ---- overlap ---------------------------------------------------------------------------------------------------------------------------
// [a, a + na) and [b, b + nb) share a byte; a NULL pointer or an empty range overlaps nothing
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}
struct Span { const void* p; size_t n; };
// no output may share a byte with an input (vs_in), nor with another output (vs_out; NULL: the outputs are not held against each other)
template <size_t NI, size_t NO> int check_spans(sarx_ctx* c, const Span (&in)[NI], const Span (&out)[NO], const char* vs_in, const char* vs_out) {
    for (size_t o = 0; o < NO; ++o) {
        for (const Span& i : in)
            if (ranges_overlap(out[o].p, out[o].n, i.p, i.n)) return fail(c, SARX_ERR_INVALID, "%s", vs_in);
        for (size_t k = o + 1; vs_out && k < NO; ++k)
            if (ranges_overlap(out[o].p, out[o].n, out[k].p, out[k].n)) return fail(c, SARX_ERR_INVALID, "%s", vs_out);
    }
    return SARX_OK;
}

// ---- the CA-CFAR's parameter block, which the OS-CFAR extends (include/sarx_gmti.h, include/sarx_oscfar.h) ---------------------------
inline int gmti_check_params(sarx_ctx* c, const sarx_gmti_params* p) {
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
inline GmtiCfarArgs gmti_cfar_args(const float* d_mag, int n_az, int n_rg, const sarx_gmti_params& p, sarx_gmti_report* d_reports,
                                   sarx_gmti_header* d_header) {
    GmtiCfarArgs a{};
    a.m = d_mag; a.n_az = n_az; a.n_rg = n_rg;
    a.ga = p.guard_az; a.gr = p.guard_rg; a.oa = p.guard_az + p.train_az; a.orr = p.guard_rg + p.train_rg;
    a.alpha = p.alpha; a.min_train = p.min_train; a.max_det = p.max_detections;
    a.rep = d_reports; a.hdr = d_header;
    return a;
}

}  // namespace sarx
