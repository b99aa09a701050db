// libsarx C ABI of include/sarx_track.h: parameter checks and the launches of track.hip.
#include "../../include/sarx_track.h"
#include "api_gmti.h"
#include "track.h"

#include <cmath>

using namespace sarx;

extern "C" {

static int track_check(sarx_ctx* c, const sarx_track_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "track params is NULL");
    if (!(p->gate_az > 0.0) || !(p->gate_rg > 0.0) || !std::isfinite(p->gate_az) || !std::isfinite(p->gate_rg))
        return fail(c, SARX_ERR_INVALID, "track gates must be finite and > 0");
    if (!(p->alpha > 0.0 && p->alpha <= 1.0)) return fail(c, SARX_ERR_INVALID, "track alpha must lie in (0, 1]");
    if (!(p->beta >= 0.0 && p->beta <= 2.0)) return fail(c, SARX_ERR_INVALID, "track beta must lie in [0, 2]");
    if (!(p->birth_ratio >= 0.0) || !std::isfinite(p->birth_ratio)) return fail(c, SARX_ERR_INVALID, "track birth_ratio must be finite and >= 0");
    if (p->confirm_window < 1 || p->confirm_window > 32 || p->confirm_hits < 1 || p->confirm_hits > p->confirm_window)
        return fail(c, SARX_ERR_INVALID, "track confirmation %d of %d: needs 1 <= hits <= window <= 32", p->confirm_hits, p->confirm_window);
    if (p->max_misses < 0) return fail(c, SARX_ERR_INVALID, "track max_misses must be >= 0");
    if (p->max_tracks < 1 || p->max_tracks > SARX_TRACK_MAX_TRACKS)
        return fail(c, SARX_ERR_INVALID, "track max_tracks %d must be 1 .. %d", p->max_tracks, SARX_TRACK_MAX_TRACKS);
    if (p->max_detections < 1 || p->max_detections > SARX_TRACK_MAX_DETECTIONS)
        return fail(c, SARX_ERR_INVALID, "track max_detections %d must be 1 .. %d", p->max_detections, SARX_TRACK_MAX_DETECTIONS);
    if (p->reserved != 0) return fail(c, SARX_ERR_INVALID, "track params: reserved must be 0");
    return SARX_OK;
}

int sarx_track_check(const sarx_track_params* p) { return track_check(nullptr, p); }

int sarx_track_table_bytes(const sarx_track_params* p, size_t* out) {
    return size_query(out, [&] { return track_check(nullptr, p); }, [&] { return table_bytes<sarx_track_header, sarx_track_slot>(p->max_tracks); });
}

int sarx_track_workspace_bytes(const sarx_track_params* p, size_t* out) {
    return size_query(out, [&] { return track_check(nullptr, p); }, [&] { return track_workspace_bytes(p->max_tracks, p->max_detections); });
}

int sarx_track_init_dev(sarx_ctx* c, const sarx_track_params* p, void* d_table) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = track_check(c, p)) return rc;
        if (const int rc = buffers_ok(c, {need(d_table, 8)}, "misaligned track table (8-byte alignment)")) return rc;
        HIPCHK(c, launch_track_init((sarx_track_header*)d_table, records_of<sarx_track_header, sarx_track_slot>(d_table), p->max_tracks, c->stream));
        return (int)SARX_OK;
    });
}

static int track_step(sarx_ctx* c, const sarx_track_params* p, const void* d_slot, int frame, void* d_table, int32_t* d_assoc_row,
                      void* d_workspace) {
    TrackArgs a{};
    a.p = *p;
    a.slot_hdr = (const sarx_gmti_header*)d_slot;
    a.rep = slot_reports(d_slot);
    a.hdr = (sarx_track_header*)d_table;
    a.slots = records_of<sarx_track_header, sarx_track_slot>(d_table);
    a.assoc = d_assoc_row;
    a.best_r = (int32_t*)d_workspace;
    a.best_t = a.best_r + track_ws_words(p->max_tracks);
    a.free_slot = a.best_t + track_ws_words(p->max_detections);
    a.frame = frame;
    HIPCHK(c, launch_track_step(a, c->stream));
    return SARX_OK;
}

static int track_buffers(sarx_ctx* c, const void* d_slots, const void* d_table, const void* d_assoc, const void* d_workspace) {
    return buffers_ok(c, {need(d_slots, 8), need(d_table, 8), need(d_workspace, 8), opt(d_assoc, 4)},
                      "misaligned slot, table, workspace (8-byte alignment) or assoc (4-byte alignment)");
}

int sarx_track_step_dev(sarx_ctx* c, const sarx_track_params* p, const void* d_slot, int frame_index, void* d_table, int32_t* d_assoc_row,
                        void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = track_check(c, p)) return rc;
        if (frame_index < 0) return fail(c, SARX_ERR_INVALID, "track frame_index must be >= 0");
        if (const int rc = track_buffers(c, d_slot, d_table, d_assoc_row, d_workspace)) return rc;
        return track_step(c, p, d_slot, frame_index, d_table, d_assoc_row, d_workspace);
    });
}

int sarx_track_run_dev(sarx_ctx* c, const sarx_track_params* p, const void* d_stack, size_t slot_stride_bytes, int n_frames, void* d_table,
                       int32_t* d_assoc, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = track_check(c, p)) return rc;
        if (n_frames < 0) return fail(c, SARX_ERR_INVALID, "track n_frames must be >= 0");
        const size_t slot = gmti_slot_bytes(p->max_detections);
        if (!stride_ok(slot_stride_bytes, slot))
            return fail(c, SARX_ERR_INVALID, "track slot stride %zu must be a multiple of 8 and at least the slot's %zu bytes", slot_stride_bytes, slot);
        if (const int rc = track_buffers(c, d_stack, d_table, d_assoc, d_workspace)) return rc;
        for (int f = 0; f < n_frames; ++f)
            if (const int rc = track_step(c, p, (const char*)d_stack + (size_t)f * slot_stride_bytes, f, d_table,
                                          d_assoc ? d_assoc + (size_t)f * p->max_detections : nullptr, d_workspace))
                return rc;
        return (int)SARX_OK;
    });
}

}  // extern "C"
