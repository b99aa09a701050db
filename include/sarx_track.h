/* libsarx GMTI tracking: a deterministic multi-target tracker over the report lists of consecutive frames.
 *
 * Plain C99.  Extends include/sarx.h and include/sarx_gmti.h (the context, the error codes and the slot layout come from there).
 *
 * Input: GMTI slots, each one sarx_gmti_header followed by max_detections sarx_gmti_report exactly as sarx_gmti_refine_dev
 * leaves them (reports sorted by (i, j)).  The report count is read from the device header: no entry point synchronises with the
 * host, no kernel uses an atomic, and ids, counters, assoc and states are the same bits from run to run and between
 * sarx_track_run_dev and the loop of sarx_track_step_dev it stands for.
 *
 * State: a table = one sarx_track_header followed by max_tracks sarx_track_slot.  A slot is free, tentative or confirmed.  A
 * track lives in pixel coordinates (i = azimuth row, j = range column): position p = (p_i, p_j), velocity v = (v_i, v_j) in
 * pixels per frame, fp64.
 *
 * One step with a frame's slot, n = count reports:
 *    1. sticky error : if the table's error field is set, the table stays as it is (the assoc row is written as -1)
 *    2. slot overflow: the slot's overflow flag set or count > max_detections: error = SARX_TRACK_ERR_SLOT_OVERFLOW, error_frame =
 *                      frame_index, the assoc row is written as -1, nothing else changes.  An overflowing list is never treated
 *                      as a truncated answer.
 *    3. predict      : for every live track ph = p + v
 *    4. distance     : d2(t, r) = ((i_r - ph_i) / gate_az)^2 + ((j_r - ph_j) / gate_rg)^2, in fp64 as two subtractions, two
 *                      divisions, two products and one sum, each rounded on its own (no fused multiply-add); eligible: d2 <= 1
 *    5. best partners: r*(t) = the eligible report of least d2 (ties: the smaller r); t*(r) = the eligible live track of least d2
 *                      (ties: the smaller slot index)
 *    6. match        : t and r are matched when r*(t) = r and t*(r) = t - ONE round of mutual nearest neighbour.  A track whose
 *                      best report prefers another track coasts this frame, even if a second report lies in its gate.
 *    7. matched      : e = z - ph;  p = ph + alpha e;  v = v + beta e;  hits += 1, misses = 0, last_frame = frame_index,
 *                      last_report = r;  sum_re += interf_re, sum_im += interf_im, sum_power += power (fp64);
 *                      max_ratio = ratio > max_ratio ? ratio : max_ratio with ratio = power / mean
 *    8. unmatched    : p = ph, misses += 1
 *    9. all live     : age += 1, hist = (hist << 1) | matched (32 bits)
 *   10. status       : tentative -> confirmed when popcount(hist & low confirm_window bits) >= confirm_hits;  then the track is
 *                      dropped when misses > max_misses, or when it is (still) tentative and age >= confirm_window.  A dropped
 *                      slot becomes free (all bytes 0) and counts in drops_total.
 *   11. births       : report r starts a track when t*(r) does not exist - no track live at the start of the step holds it in its
 *                      gate, so it is not matched either - and (birth_ratio = 0 or power / mean >= birth_ratio).  Such reports
 *                      in rising r take the free slots in rising slot index (slots freed in this step included) and the ids
 *                      next_id, next_id + 1, ...: p = z, v = 0, tentative, hits = 1, misses = 0, hist = 1, age = 1, sums and
 *                      max_ratio from the report.  More births than free slots: error = SARX_TRACK_ERR_TABLE_OVERFLOW,
 *                      error_frame = frame_index, NO birth is made and their assoc entries stay -1 (steps 3 - 10 stand).
 *                      No partial birth list is ever presented as complete.
 *   12. assoc        : assoc[r] = id of the matched or born track, else -1; all max_detections entries are written, -1 past n.
 *   A step that ends without an error adds one to frames_done; n_live and n_confirmed are counted anew in every step that gets
 *   past 2.
 *
 * A report inside the gate of a track that did not take it starts nothing: that suppresses duplicate tracks beside a real one,
 * at the price of a late birth for a close neighbour (it is born once the neighbour's gate no longer holds it).
 *
 * Tracking in ground coordinates: sarx_relocate.h makes the slots of this tracker from a frame's reports and their radial
 * speeds, on a ground grid of the caller's choosing; the pixels here are then that grid's.
 *
 * Left out: a Kalman covariance (sarx_ktrack.h has one, for reports relocated to the ground: metres, a Mahalanobis gate, the radial
 * speed as a measurement), multi-hypothesis or globally optimal assignment, and feeding the track velocity back into the refocus
 * grid. */
#ifndef SARX_TRACK_H
#define SARX_TRACK_H

#include "sarx.h"
#include "sarx_gmti.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_TRACK_MAX_TRACKS 16384
#define SARX_TRACK_MAX_DETECTIONS 65536

enum { SARX_TRACK_FREE = 0, SARX_TRACK_TENTATIVE = 1, SARX_TRACK_CONFIRMED = 2 };
enum { SARX_TRACK_OK = 0, SARX_TRACK_ERR_SLOT_OVERFLOW = 1, SARX_TRACK_ERR_TABLE_OVERFLOW = 2 };

typedef struct {
    double gate_az, gate_rg;       /* gate half-widths in pixels (> 0) */
    double alpha;                  /* position gain, 0 < alpha <= 1 */
    double beta;                   /* velocity gain, 0 <= beta <= 2 */
    double birth_ratio;            /* >= 0; 0 = every report may start a track */
    int32_t confirm_hits;          /* M: 1 <= M <= N */
    int32_t confirm_window;        /* N <= 32 */
    int32_t max_misses;            /* >= 0 */
    int32_t max_tracks;            /* 1 .. SARX_TRACK_MAX_TRACKS */
    int32_t max_detections;        /* capacity of the slots, 1 .. SARX_TRACK_MAX_DETECTIONS */
    int32_t reserved;              /* 0 */
} sarx_track_params;               /* 64 bytes */

typedef struct {
    uint32_t n_live;               /* tentative + confirmed */
    uint32_t n_confirmed;
    int32_t next_id;               /* ids start at 0 */
    uint32_t frames_done;          /* steps finished without an error */
    uint32_t births_total;
    uint32_t drops_total;
    uint32_t error;                /* SARX_TRACK_OK, _ERR_SLOT_OVERFLOW or _ERR_TABLE_OVERFLOW; sticky */
    int32_t error_frame;           /* frame_index of the step that set it, -1 without an error */
    uint32_t max_tracks;
    uint32_t reserved[7];          /* 0 */
} sarx_track_header;               /* 64 bytes */

typedef struct {
    double p_i, p_j;               /* position, pixels */
    double v_i, v_j;               /* velocity, pixels per frame */
    double sum_re, sum_im;         /* sum of the matched reports' interferograms */
    double sum_power;              /* sum of their power */
    double max_ratio;              /* largest power / mean among them */
    int32_t id;
    uint32_t status;               /* SARX_TRACK_FREE / _TENTATIVE / _CONFIRMED */
    uint32_t hits, misses;         /* reports taken in all; consecutive frames without one */
    uint32_t age;                  /* steps lived, the birth counts */
    uint32_t hist;                 /* bit k: matched k steps ago */
    int32_t last_frame, last_report;
} sarx_track_slot;                 /* 96 bytes */

/* validates the parameters (no device needed) */
int sarx_track_check(const sarx_track_params* params);
/* bytes of the table (header + max_tracks slots) and of the workspace (content not defined) */
int sarx_track_table_bytes(const sarx_track_params* params, size_t* out_bytes);
int sarx_track_workspace_bytes(const sarx_track_params* params, size_t* out_bytes);
/* an empty table: every byte of it is written (d_table 8-byte aligned, as everywhere below) */
int sarx_track_init_dev(sarx_ctx* ctx, const sarx_track_params* params, void* d_table);
/* one step with the slot at d_slot (8-byte aligned).  d_assoc_row: max_detections int32 (4-byte aligned) or NULL.  Two launches on
 * the ctx's current lane. */
int sarx_track_step_dev(sarx_ctx* ctx, const sarx_track_params* params, const void* d_slot, int frame_index, void* d_table,
                        int32_t* d_assoc_row, void* d_workspace);
/* steps frame_index = 0 .. n_frames - 1 over the slots at d_stack + f slot_stride_bytes (the stride a multiple of 8 and at least
 * the slot's size: records behind the reports are skipped).  d_assoc: [n_frames x max_detections] int32 or NULL.  Only enqueues,
 * on the ctx's current lane. */
int sarx_track_run_dev(sarx_ctx* ctx, const sarx_track_params* params, const void* d_stack, size_t slot_stride_bytes, int n_frames,
                       void* d_table, int32_t* d_assoc, void* d_workspace);

#ifdef __cplusplus
}
#endif
#endif /* SARX_TRACK_H */
