// libsarx C ABI of include/sarx_ktrack.h: parameter checks and the launches of ktrack.hip.
#include "../../include/sarx_ktrack.h"
#include "api_gmti.h"
#include "ktrack.h"

#include <cmath>

using namespace sarx;

static int ktrack_check(sarx_ctx* c, const sarx_ktrack_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "ktrack params is NULL");
    const struct { const char* name; double v; bool zero_ok; } f[] = {
        {"sigma_pos", p->sigma_pos, false}, {"sigma_v", p->sigma_v, false}, {"sigma_v_tan", p->sigma_v_tan, false}, {"q", p->q, true},
        {"gate_d2", p->gate_d2, false},     {"gate_m", p->gate_m, false},   {"birth_ratio", p->birth_ratio, true}};
    for (const auto& x : f)
        if (!std::isfinite(x.v) || !(x.zero_ok ? x.v >= 0.0 : x.v > 0.0))
            return fail(c, SARX_ERR_INVALID, "ktrack %s must be finite and %s 0", x.name, x.zero_ok ? ">=" : ">");
    if (p->confirm_window < 1 || p->confirm_window > 32)
        return fail(c, SARX_ERR_INVALID, "ktrack confirm_window %d must be 1 .. 32", p->confirm_window);
    if (p->confirm_hits < 1 || p->confirm_hits > p->confirm_window)
        return fail(c, SARX_ERR_INVALID, "ktrack confirm_hits %d must be 1 .. confirm_window = %d", p->confirm_hits, p->confirm_window);
    if (p->max_misses < 0) return fail(c, SARX_ERR_INVALID, "ktrack max_misses must be >= 0");
    if (p->max_tracks < 1 || p->max_tracks > SARX_KTRACK_MAX_TRACKS)
        return fail(c, SARX_ERR_INVALID, "ktrack max_tracks %d must be 1 .. %d", p->max_tracks, SARX_KTRACK_MAX_TRACKS);
    if (p->max_detections < 1 || p->max_detections > SARX_KTRACK_MAX_DETECTIONS)
        return fail(c, SARX_ERR_INVALID, "ktrack max_detections %d must be 1 .. %d", p->max_detections, SARX_KTRACK_MAX_DETECTIONS);
    if (p->reserved != 0) return fail(c, SARX_ERR_INVALID, "ktrack params: reserved must be 0");
    return SARX_OK;
}

static int ktrack_frame_check(sarx_ctx* c, const sarx_ktrack_frame* f) {
    if (!f) return fail(c, SARX_ERR_INVALID, "ktrack frame is NULL");
    if (!std::isfinite(f->t)) return fail(c, SARX_ERR_INVALID, "ktrack frame: t must be finite");
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(f->pos_ref[k])) return fail(c, SARX_ERR_INVALID, "ktrack frame: pos_ref[%d] must be finite", k);
        if (!std::isfinite(f->vel_ref[k])) return fail(c, SARX_ERR_INVALID, "ktrack frame: vel_ref[%d] must be finite", k);
    }
    if (f->frame_index < 0) return fail(c, SARX_ERR_INVALID, "ktrack frame: frame_index must be >= 0");
    if (f->reserved != 0) return fail(c, SARX_ERR_INVALID, "ktrack frame: reserved must be 0");
    return SARX_OK;
}

// the extent of one frame's v_los array: max_detections elements at the stride
static size_t v_los_extent(size_t stride, size_t md) { return (md - 1) * stride + 8; }

static int ktrack_buffers(sarx_ctx* c, const sarx_ktrack_params* p, const void* d_slots, size_t slots_bytes, const void* d_records,
                          size_t records_bytes, const void* d_v_los, size_t v_los_bytes, const void* d_table, const void* d_assoc,
                          size_t assoc_bytes, const void* d_workspace) {
    if (const int rc = buffers_ok(c, {need(d_slots, 8), need(d_records, 8), need(d_v_los, 8), need(d_table, 8), need(d_workspace, 8), opt(d_assoc, 4)},
                                  "misaligned slot, records, v_los, table, workspace (8-byte alignment) or assoc (4-byte alignment)"))
        return rc;
    const Span in[] = {{d_slots, slots_bytes}, {d_records, records_bytes}, {d_v_los, v_los_bytes}};
    const Span out[] = {{d_table, table_bytes<sarx_ktrack_header, sarx_ktrack_slot>(p->max_tracks)},
                        {d_workspace, ktrack_workspace_bytes(p->max_tracks, p->max_detections)},
                        {d_assoc, assoc_bytes}};
    return check_spans(c, in, out, "the ktrack table, workspace or assoc overlap an input", "the ktrack table, workspace and assoc overlap each other");
}

static int ktrack_step(sarx_ctx* c, const sarx_ktrack_params* p, const sarx_ktrack_frame* f, const void* d_slot, const void* d_records,
                       const void* d_v_los, size_t v_los_stride, void* d_table, int32_t* d_assoc_row, void* d_workspace) {
    KtrackArgs a{};
    a.p = *p;
    a.f = *f;
    a.slot_hdr = (const sarx_gmti_header*)d_slot;
    a.rep = slot_reports(d_slot);
    a.rec = (const sarx_relocate_record*)d_records;
    a.v_los = (const char*)d_v_los;
    a.v_los_stride = v_los_stride;
    a.hdr = (sarx_ktrack_header*)d_table;
    a.slots = records_of<sarx_ktrack_header, sarx_ktrack_slot>(d_table);
    a.assoc = d_assoc_row;
    a.tp = (int)ktrack_padded(p->max_tracks);
    a.rp = (int)ktrack_padded(p->max_detections);
    a.pred = (double*)d_workspace;
    a.nis = a.pred + (size_t)KTRACK_PRED * a.tp;
    a.meas = a.nis + a.tp;
    a.best_r = (int32_t*)(a.meas + (size_t)KTRACK_MEAS * a.rp);
    a.best_t = a.best_r + a.tp;
    a.free_slot = a.best_t + a.rp;
    HIPCHK(c, launch_ktrack_step(a, c->stream));
    return SARX_OK;
}

extern "C" {

int sarx_ktrack_check(const sarx_ktrack_params* p) { return ktrack_check(nullptr, p); }

int sarx_ktrack_table_bytes(const sarx_ktrack_params* p, size_t* out) {
    return size_query(out, [&] { return ktrack_check(nullptr, p); }, [&] { return table_bytes<sarx_ktrack_header, sarx_ktrack_slot>(p->max_tracks); });
}

int sarx_ktrack_workspace_bytes(const sarx_ktrack_params* p, size_t* out) {
    return size_query(out, [&] { return ktrack_check(nullptr, p); }, [&] { return ktrack_workspace_bytes(p->max_tracks, p->max_detections); });
}

int sarx_ktrack_init_dev(sarx_ctx* c, const sarx_ktrack_params* p, void* d_table) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = ktrack_check(c, p)) return rc;
        if (const int rc = buffers_ok(c, {need(d_table, 8)}, "misaligned ktrack table (8-byte alignment)")) return rc;
        HIPCHK(c, launch_ktrack_init((sarx_ktrack_header*)d_table, records_of<sarx_ktrack_header, sarx_ktrack_slot>(d_table), p->max_tracks, c->stream));
        return (int)SARX_OK;
    });
}

int sarx_ktrack_step_dev(sarx_ctx* c, const sarx_ktrack_params* p, const sarx_ktrack_frame* f, const void* d_slot, const void* d_records,
                         const void* d_v_los, size_t v_los_stride, void* d_table, int32_t* d_assoc_row, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = ktrack_check(c, p)) return rc;
        if (const int rc = ktrack_frame_check(c, f)) return rc;
        if (!stride_ok(v_los_stride, 8)) return fail(c, SARX_ERR_INVALID, "ktrack v_los_stride %zu must be a multiple of 8, >= 8", v_los_stride);
        const size_t md = (size_t)p->max_detections;
        if (const int rc = ktrack_buffers(c, p, d_slot, gmti_slot_bytes(p->max_detections), d_records, md * sizeof(sarx_relocate_record), d_v_los,
                                          v_los_extent(v_los_stride, md), d_table, d_assoc_row, md * sizeof(int32_t), d_workspace))
            return rc;
        return ktrack_step(c, p, f, d_slot, d_records, d_v_los, v_los_stride, d_table, d_assoc_row, d_workspace);
    });
}

int sarx_ktrack_run_dev(sarx_ctx* c, const sarx_ktrack_params* p, const sarx_ktrack_frame* frames, int n_frames, const void* d_slots,
                        size_t slot_stride, const void* d_records, size_t records_stride, const void* d_v_los, size_t v_los_stride,
                        size_t v_los_frame_stride, void* d_table, int32_t* d_assoc, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = ktrack_check(c, p)) return rc;
        if (n_frames < 0) return fail(c, SARX_ERR_INVALID, "ktrack n_frames must be >= 0");
        if (n_frames > 0 && !frames) return fail(c, SARX_ERR_INVALID, "ktrack frames is NULL");
        for (int f = 0; f < n_frames; ++f)
            if (const int rc = ktrack_frame_check(c, frames + f)) return rc;
        const size_t md = (size_t)p->max_detections, slot = gmti_slot_bytes(p->max_detections), recs = md * sizeof(sarx_relocate_record);
        if (!stride_ok(v_los_stride, 8)) return fail(c, SARX_ERR_INVALID, "ktrack v_los_stride %zu must be a multiple of 8, >= 8", v_los_stride);
        const size_t speeds = v_los_extent(v_los_stride, md);
        if (!stride_ok(slot_stride, slot))
            return fail(c, SARX_ERR_INVALID, "ktrack slot_stride %zu must be a multiple of 8 and at least the slot's %zu bytes", slot_stride, slot);
        if (!stride_ok(records_stride, recs))
            return fail(c, SARX_ERR_INVALID, "ktrack records_stride %zu must be a multiple of 8 and at least the records' %zu bytes", records_stride, recs);
        if (!stride_ok(v_los_frame_stride, speeds))
            return fail(c, SARX_ERR_INVALID, "ktrack v_los_frame_stride %zu must be a multiple of 8 and at least the speeds' %zu bytes",
                        v_los_frame_stride, speeds);
        const size_t last = n_frames > 0 ? (size_t)(n_frames - 1) : 0, nf = (size_t)(n_frames > 0 ? 1 : 0);
        if (const int rc = ktrack_buffers(c, p, d_slots, nf * (last * slot_stride + slot), d_records, nf * (last * records_stride + recs), d_v_los,
                                          nf * (last * v_los_frame_stride + speeds), d_table, d_assoc, (size_t)n_frames * md * sizeof(int32_t),
                                          d_workspace))
            return rc;
        for (int f = 0; f < n_frames; ++f)
            if (const int rc = ktrack_step(c, p, frames + f, (const char*)d_slots + (size_t)f * slot_stride, (const char*)d_records + (size_t)f * records_stride,
                                           (const char*)d_v_los + (size_t)f * v_los_frame_stride, v_los_stride, d_table,
                                           d_assoc ? d_assoc + (size_t)f * md : nullptr, d_workspace))
                return rc;
        return (int)SARX_OK;
    });
}

}  // extern "C"
