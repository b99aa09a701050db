/* libsarx ground tracking of GMTI reports: a Kalman filter per track over relocated reports and their radial speeds
 * (DESIGN.md 4.22).
 *
 * Plain C99.  Extends include/sarx.h, include/sarx_gmti.h and include/sarx_relocate.h (the context, the error codes, the slot
 * layout and the relocation's record come from there); the limits of the table are those of include/sarx_track.h, the limit of
 * the report lists that of include/sarx_tdbp_multi.h.
 *
 * What it is for.  sarx_relocate.h puts a report at g = P_xy + al a + ..., al = (w.V + v_los R) / |V_xy|: an error e_v of the
 * radial speed moves the report k e_v ALONG TRACK, k = R / |V_xy| (27 s on a 5 km circle, 66 s on the orbit arc), against about a
 * pixel across.  The error of a relocated position is an ellipse that turns with the aspect angle, it is correlated with the
 * error of v_los, and v_los itself measures one component of the ground velocity.  The tracker of sarx_track.h (integer pixels, a
 * fixed box gate, fixed gains, velocity from position differences) knows none of that; this one carries a state (x, y, vx, vy)
 * in metres and m/s with its 4 x 4 covariance P, gates on the Mahalanobis distance of (x, y, v_los) and starts a track with the
 * velocity component the first report measures.
 *
 * Input of a step, all on the device, as ONE call of sarx_relocate_dev left it: the relocation's INPUT slot (the report payload
 * and the count n), its record array (record r belongs to input report r) and the v_los array it read, at its stride (the
 * resolver's records go in at stride 64).  The count is read from the device header: no entry point synchronises with the host,
 * no kernel uses an atomic, every fp64 value is computed by exactly one thread, and ids, counters, assoc and states are the same
 * bits from run to run and between sarx_ktrack_run_dev and the loop of sarx_ktrack_step_dev it stands for.
 *
 * Arithmetic.  Everything is fp64; every operation written below is one IEEE operation rounded on its own (no fused multiply-add),
 * sums and products are taken left to right as written, brackets first.  tests/_ktrack_numpy.py restates them in this order.
 *
 * Table: one sarx_ktrack_header, then max_tracks sarx_ktrack_slot.  P is kept as its upper triangle, row-major over the state
 * order (x, y, vx, vy): p[0..9] = P00 P01 P02 P03 P11 P12 P13 P22 P23 P33; below, Pij with i > j means Pji.
 *
 * One step with a frame (t, P = pos_ref, V = vel_ref, frame_index), n = the slot's count:
 *    1. errors   : a. sticky: if the table's error field is set, the table stays as it is (the assoc row is written as -1).
 *                  b. slot overflow: the slot's overflow flag set, n > max_detections, or (n >= 1 and) record 0 with status
 *                     SARX_RELOCATE_OVERFLOW: error = SARX_KTRACK_ERR_SLOT_OVERFLOW, error_frame = frame_index, the assoc row is
 *                     written as -1, nothing else changes.  An overflowing list is never treated as a truncated answer.
 *                  c. time: dt = 0 on the first step of a table (frames_done = 0), else dt = t - t_last.  dt < 0 or not finite:
 *                     error = SARX_KTRACK_ERR_TIME, error_frame = frame_index, assoc row -1, nothing else changes.
 *    2. predict  : for every live track, with dt2 = dt dt, dt3 = dt2 dt, q11 = q (dt3 / 3), q13 = q (dt2 / 2), q33 = q dt:
 *                     x- = x + dt vx;  y- = y + dt vy;  vx- = vx;  vy- = vy                       (F = [[I, dt I], [0, I]])
 *                     P00- = P00 + dt (P02 + P02) + dt2 P22 + q11      P01- = P01 + dt (P03 + P12) + dt2 P23
 *                     P11- = P11 + dt (P13 + P13) + dt2 P33 + q11      P02- = P02 + dt P22 + q13
 *                     P03- = P03 + dt P23      P12- = P12 + dt P23     P13- = P13 + dt P33 + q13
 *                     P22- = P22 + q33         P23- = P23              P33- = P33 + q33           (P- = F P F' + Q)
 *    3. measure  : report r < n is a measurement when its record's status is SARX_RELOCATE_OK or _OFF_GRID (both are solved; this
 *                  tracker has no grid), v = v_los[r] and the record's g = (x, y) are finite, s != 0 and rho2 != 0 below:
 *                     s = sqrt(V_x V_x + V_y V_y);  a = (V_x / s, V_y / s);  n = (-a_y, a_x)
 *                     d = (g_x - P_x, g_y - P_y);  rho2 = d_x d_x + d_y d_y;  R = sqrt(rho2 + P_z P_z)
 *                     u = (d_x / R, d_y / R)           relocate's u; NOT a unit vector: |u| = sqrt(rho2) / R
 *                     k = R / s;  ka = (k a_x, k a_y);  sp2 = sigma_pos sigma_pos;  sv2 = sigma_v sigma_v
 *                     z = (g_x, g_y, v);  H = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, u_x, u_y]]   (linear: u at the measured position)
 *                     Rm = J diag(sp2, sp2, sv2) J', J's columns (a, 0), (n, 0), (ka, 1): along-track placement, cross-track
 *                     placement and speed error, the last moving the report k e_v along track:
 *                     Rm00 = (a_x a_x) sp2 + (n_x n_x) sp2 + (ka_x ka_x) sv2      Rm02 = ka_x sv2
 *                     Rm01 = (a_x a_y) sp2 + (n_x n_y) sp2 + (ka_x ka_y) sv2      Rm12 = ka_y sv2
 *                     Rm11 = (a_y a_y) sp2 + (n_y n_y) sp2 + (ka_y ka_y) sv2      Rm22 = sv2
 *    4. distance : per track and measurement, nu = z - H x-:
 *                     nu_x = z_x - x-;  nu_y = z_y - y-;  nu_v = z_v - (u_x vx- + u_y vy-)
 *                     c_i = u_x P-[i][2] + u_y P-[i][3], i = 0 .. 3                              (the third column of P- H')
 *                     S00 = P00- + Rm00;  S01 = P01- + Rm01;  S11 = P11- + Rm11;  S02 = c_0 + Rm02;  S12 = c_1 + Rm12
 *                     S22 = (u_x c_2 + u_y c_3) + Rm22                                            (S = H P- H' + Rm)
 *                  S = L L' without pivoting, then w = L^-1 nu:
 *                     l00 = sqrt(S00);  l10 = S01 / l00;  l20 = S02 / l00;  l11 = sqrt(S11 - l10 l10)
 *                     l21 = (S12 - l20 l10) / l11;  l22 = sqrt((S22 - l20 l20) - l21 l21)
 *                     w_0 = nu_x / l00;  w_1 = (nu_y - l10 w_0) / l11;  w_2 = ((nu_v - l20 w_0) - l21 w_1) / l22
 *                     d2 = (w_0 w_0 + w_1 w_1) + w_2 w_2
 *                  eligible: |nu_x| <= gate_m and |nu_y| <= gate_m and d2 <= gate_d2 (a comparison with a NaN fails).  gate_m is
 *                  part of the decision, not only a way to skip the factorisation.
 *    5. partners : r*(t) = the eligible measurement of least d2 (ties: the smaller r); t*(r) = the eligible live track of least d2
 *                  (ties: the smaller slot index).  t and r are matched when r*(t) = r and t*(r) = t: ONE round of mutual nearest
 *                  neighbour, as sarx_track.h steps 5 and 6.
 *    6. matched  : with row i of P- H' = (P-[i][0], P-[i][1], c_i) = (b_0, b_1, b_2), row i of K = P- H' S^-1 by the same factor:
 *                     y_0 = b_0 / l00;  y_1 = (b_1 - l10 y_0) / l11;  y_2 = ((b_2 - l20 y_0) - l21 y_1) / l22
 *                     K_i2 = y_2 / l22;  K_i1 = (y_1 - l21 K_i2) / l11;  K_i0 = ((y_0 - l10 K_i1) - l20 K_i2) / l00
 *                     state_i = state_i- + ((K_i0 nu_x + K_i1 nu_y) + K_i2 nu_v)
 *                  A = I - K H:  A_i0 = [i = 0] - K_i0;  A_i1 = [i = 1] - K_i1;  A_i2 = [i = 2] - K_i2 u_x;  A_i3 = [i = 3] - K_i2 u_y
 *                     M_ij = ((A_i0 P-[0][j] + A_i1 P-[1][j]) + A_i2 P-[2][j]) + A_i3 P-[3][j]                  (M = A P-)
 *                     G_ic = (K_i0 Rm[0][c] + K_i1 Rm[1][c]) + K_i2 Rm[2][c]                                     (G = K Rm)
 *                     for j >= i:  T = ((M_i0 A_j0 + M_i1 A_j1) + M_i2 A_j2) + M_i3 A_j3
 *                                  U = (G_i0 K_j0 + G_i1 K_j1) + G_i2 K_j2;   P[i][j] = T + U              (Joseph form)
 *                  nis_last = d2;  nis_sum = nis_sum + d2;  hits += 1, misses = 0, last_frame = frame_index, last_report = r;
 *                  sum_re, sum_im, sum_power, max_ratio from the slot's report r as sarx_track.h step 7.
 *    7. unmatched: state = state-, P = P-, misses += 1
 *    8. all live : age, hist, confirmation and drops: sarx_track.h steps 9 and 10, unchanged.
 *    9. births   : measurement r starts a track when t*(r) does not exist and (birth_ratio = 0 or power / mean >= birth_ratio);
 *                  the order of free slots and ids and the all-or-nothing table overflow (SARX_KTRACK_ERR_TABLE_OVERFLOW) are
 *                  sarx_track.h step 11.  The new track: tentative, hits = 1, misses = 0, hist = 1, age = 1, nis_last = nis_sum =
 *                  0, sums and max_ratio from the report, (x, y) = g, and with
 *                     m = sqrt(u_x u_x + u_y u_y);  e = (u_x / m, u_y / m);  em = (e_x / m, e_y / m);  tn = (-e_y, e_x)
 *                     vr = v / m;  (vx, vy) = (vr e_x, vr e_y)                     (H x = z: the radial component is the report's.
 *                                                                                   v u instead would be short by the factor m m)
 *                     P00 = Rm00;  P01 = Rm01;  P11 = Rm11                         (the position block of Rm)
 *                     P02 = Rm02 em_x;  P03 = Rm02 em_y;  P12 = Rm12 em_x;  P13 = Rm12 em_y       (k sv2 a (e / m)')
 *                     sm = sigma_v / m;  sm2 = sm sm;  st2 = sigma_v_tan sigma_v_tan
 *                     P22 = sm2 (e_x e_x) + st2 (tn_x tn_x);  P23 = sm2 (e_x e_y) + st2 (tn_x tn_y)
 *                     P33 = sm2 (e_y e_y) + st2 (tn_y tn_y)
 *                  When the record has SARX_RELOCATE_HAS_VELOCITY: (vx, vy) = the record's, P22 = P33 = sv2, P23 = 0, the rest
 *                  as above.
 *   10. assoc    : assoc[r] = id of the matched or born track, else -1, indexed by the input report r; all max_detections entries
 *                  are written, -1 past n.
 *   11. end      : t_last = t; a step that ends without an error adds one to frames_done; n_live and n_confirmed are counted anew
 *                  in every step that gets past 1.  (A table overflow leaves steps 2 - 8 and t_last = t standing.)
 *
 * A report that is no measurement starts nothing and is matched with nothing.  A measurement inside the gate of a track that did
 * not take it starts nothing either, as in sarx_track.h.
 *
 * Left out: manoeuvre models (IMM), multi-hypothesis or globally optimal assignment, the birth covariance when a full velocity is
 * given (sv2 I is a placeholder: the pair search's along-track speed has an error of its own, and the position-velocity block is
 * kept as if only v_los were known), terrain height (the ground is z = 0, as in sarx_relocate.h), and feeding the track's velocity
 * back into the pair search's hypotheses. */
#ifndef SARX_KTRACK_H
#define SARX_KTRACK_H

#include "sarx.h"
#include "sarx_gmti.h"
#include "sarx_relocate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_KTRACK_MAX_TRACKS 16384        /* SARX_TRACK_MAX_TRACKS */
#define SARX_KTRACK_MAX_DETECTIONS 16384    /* SARX_TDBP_MULTI_MAX_DETECTIONS */

enum { SARX_KTRACK_FREE = 0, SARX_KTRACK_TENTATIVE = 1, SARX_KTRACK_CONFIRMED = 2 };
enum { SARX_KTRACK_OK = 0, SARX_KTRACK_ERR_SLOT_OVERFLOW = 1, SARX_KTRACK_ERR_TABLE_OVERFLOW = 2, SARX_KTRACK_ERR_TIME = 3 };

typedef struct {
    double sigma_pos;              /* m, finite and > 0: placement error of a report, per axis */
    double sigma_v;                /* m/s, finite and > 0: error of v_los */
    double sigma_v_tan;            /* m/s, finite and > 0: prior of the velocity component the first report does not measure */
    double q;                      /* m^2/s^3, finite and >= 0: white-acceleration density */
    double gate_d2;                /* finite and > 0: gate on the Mahalanobis distance squared, 3 degrees of freedom */
    double gate_m;                 /* m, finite and > 0: half-width of the coarse box on (nu_x, nu_y) */
    double birth_ratio;            /* finite and >= 0; 0 = every measurement may start a track */
    int32_t confirm_hits;          /* M: 1 <= M <= N */
    int32_t confirm_window;        /* N <= 32 */
    int32_t max_misses;            /* >= 0 */
    int32_t max_tracks;            /* 1 .. SARX_KTRACK_MAX_TRACKS */
    int32_t max_detections;        /* capacity of the slot, the records and v_los, 1 .. SARX_KTRACK_MAX_DETECTIONS */
    int32_t reserved;              /* 0 */
} sarx_ktrack_params;              /* 80 bytes */

typedef struct {
    double t;                      /* s, finite: the frame's reference time */
    double pos_ref[3], vel_ref[3]; /* finite: what the frame's sarx_relocate_params carried */
    int32_t frame_index;           /* >= 0 */
    int32_t reserved;              /* 0 */
} sarx_ktrack_frame;               /* 64 bytes */

typedef struct {
    uint32_t n_live;               /* tentative + confirmed */
    uint32_t n_confirmed;
    int32_t next_id;               /* ids start at 0 */
    uint32_t frames_done;          /* steps finished without an error */
    uint32_t births_total;
    uint32_t drops_total;
    uint32_t error;                /* SARX_KTRACK_OK or one of SARX_KTRACK_ERR_*; sticky */
    int32_t error_frame;           /* frame_index of the step that set it, -1 without an error */
    uint32_t max_tracks;
    uint32_t reserved0;            /* 0 */
    double t_last;                 /* t of the last step that got past 1 */
    uint32_t reserved[4];          /* 0 */
} sarx_ktrack_header;              /* 64 bytes */

typedef struct {
    double x, y;                   /* position, m */
    double vx, vy;                 /* ground velocity, m/s */
    double p[10];                  /* upper triangle of P: P00 P01 P02 P03 P11 P12 P13 P22 P23 P33 */
    double sum_re, sum_im;         /* sum of the matched reports' interferograms */
    double sum_power;              /* sum of their power */
    double max_ratio;              /* largest power / mean among them */
    double nis_last;               /* d2 of the last match, 0 before the first */
    double nis_sum;                /* sum of d2 over the matches: nis_sum / (hits - 1) is the mean */
    int32_t id;
    uint32_t status;               /* SARX_KTRACK_FREE / _TENTATIVE / _CONFIRMED */
    uint32_t hits, misses;         /* reports taken in all; consecutive frames without one */
    uint32_t age;                  /* steps lived, the birth counts */
    uint32_t hist;                 /* bit k: matched k steps ago */
    int32_t last_frame, last_report;
} sarx_ktrack_slot;                /* 192 bytes */

/* validates the parameters (no device needed): SARX_OK, or SARX_ERR_INVALID and a message naming the field in sarx_last_error(NULL) */
int sarx_ktrack_check(const sarx_ktrack_params* params);
/* bytes of the table (header + max_tracks slots) and of the workspace (content not defined) */
int sarx_ktrack_table_bytes(const sarx_ktrack_params* params, size_t* out_bytes);
int sarx_ktrack_workspace_bytes(const sarx_ktrack_params* params, size_t* out_bytes);
/* an empty table: every byte of it is written (d_table 8-byte aligned, as everywhere below) */
int sarx_ktrack_init_dev(sarx_ctx* ctx, const sarx_ktrack_params* params, void* d_table);
/* one step.  d_slot: the relocation's input slot; d_records: its max_detections sarx_relocate_record; d_v_los: fp64 per report,
 * v_los_stride bytes apart (a multiple of 8, >= 8) - all 8-byte aligned, read only up to the slot's count.  d_assoc_row:
 * max_detections int32 (4-byte aligned) or NULL; d_workspace 8-byte aligned.  Table, workspace and assoc row may overlap no input and
 * not each other.  Four launches on the ctx's current lane. */
int sarx_ktrack_step_dev(sarx_ctx* ctx, const sarx_ktrack_params* params, const sarx_ktrack_frame* frame, const void* d_slot,
                         const void* d_records, const void* d_v_los, size_t v_los_stride, void* d_table, int32_t* d_assoc_row,
                         void* d_workspace);
/* steps over frames[0 .. n_frames - 1] (a host array, read before the call returns), frame f with the slot at d_slots + f
 * slot_stride, the records at d_records + f records_stride and the speeds at d_v_los + f v_los_frame_stride (every stride in
 * bytes, a multiple of 8 and at least one frame's extent: sarx.relocate_frames lays slots and records out so).  d_assoc:
 * [n_frames x max_detections] int32 or NULL.  Only enqueues, on the ctx's current lane. */
int sarx_ktrack_run_dev(sarx_ctx* ctx, const sarx_ktrack_params* params, const sarx_ktrack_frame* frames, int n_frames,
                        const void* d_slots, size_t slot_stride, const void* d_records, size_t records_stride, const void* d_v_los,
                        size_t v_los_stride, size_t v_los_frame_stride, void* d_table, int32_t* d_assoc, void* d_workspace);

#ifdef __cplusplus
}
#endif
#endif /* SARX_KTRACK_H */
