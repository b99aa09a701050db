/* libsarx ground relocation of GMTI reports.
 *
 * A mover is imaged at the ground point whose range and range rate match its own: hundreds of metres along track from where
 * it is.  With its radial speed v_los (sarx_tdbp_pair.h, the resolver of sarx_tdbp_multi.h) that is undone: each report of a
 * GMTI slot gets the ground position at the same range whose range rate is less by v_los, and the reports that land on the
 * caller's output grid make a GMTI slot again, which the tracker (sarx_track.h) and the plot extraction (sarx_cluster.h) take
 * unchanged - in ground coordinates, where a steady mover moves v dt per frame whatever the aspect angle.
 *
 * Semantics.  Everything is fp64; the count is read from the input slot's header on the device (no host round trip); two
 * launches on the ctx's current lane, only enqueued; no atomics: the same bits from run to run.  Per report r at pixel (i, j):
 *     q     = (in_x0 + j in_dx, in_y0 + i in_dy, 0)        image position (the grid of sarx_tdbp_*: x0 = y0 = -S / 2,
 *                                                          dx = S / (nx - 1), dy = S / (ny - 1))
 *     P, V  = pos_ref, vel_ref                             phase centre and its velocity at the CPI's reference time
 *     w     = q - P;  h = -P_z;  rho2 = w_x^2 + w_y^2;  R = sqrt(rho2 + h^2)
 *     s2    = V_x^2 + V_y^2;  a = (V_x, V_y) / sqrt(s2);  n = (-a_y, a_x)
 *     c     = w_x V_x + w_y V_y + v_los R                  (= w.V + v_los R - h V_z: the mover's range rate at g is that of a
 *                                                          still point at q)
 *     al    = c / sqrt(s2);  h2 = rho2 - al^2
 *     side  = +1 if w_x n_x + w_y n_y >= 0 else -1         the mover lies on the image's side of the track
 *     g     = (P_x, P_y) + al a + side sqrt(h2) n          same range as q, range rate less v_los: circle and line on z = 0
 * v_los (d_v_los, one fp64 per report, v_los_stride bytes apart) is positive for a receding target: the sign of the pair's and
 * of the resolver's v_los.
 *
 * Record r (64 bytes): x, y = g;  shift_x, shift_y = g - q;  rank = the report's index in the output slot or -1;  status;
 * vx, vy and flags, the ground velocity:
 *     computed when d_v_along is not NULL and its value for the report is finite: v_along is the target's ground speed along
 *     a (the pair search's estimate when its hypotheses run along track).  With u = ((g_x - P_x) / R, (g_y - P_y) / R),
 *         vx u_x + vy u_y = v_los,   vx a_x + vy a_y = v_along
 *         det = u_x a_y - u_y a_x;   vx = (v_los a_y - u_y v_along) / det;   vy = (u_x v_along - a_x v_los) / det
 *     flags bit 0 (SARX_RELOCATE_HAS_VELOCITY) is set when det is non-zero and vx, vy are finite; else vx = vy = 0, bit clear.
 * status, the first that applies:
 *     SARX_RELOCATE_NO_SPEED     d_valid not NULL and the report's word (uint32, valid_stride bytes apart) non-zero, or v_los not
 *                                finite.  With d_valid = &record[0].status of the resolver's records, d_v_los = the records
 *                                and both strides 64, the resolver's output goes in as it lies on the device.
 *     SARX_RELOCATE_NO_SOLUTION  s2 == 0, rho2 <= 0, or h2 < 0 or not a number: no ground point at that range has that Doppler.
 *     SARX_RELOCATE_OFF_GRID     solved (x, y, shift, vx, vy, flags as above), but the nearest output pixel
 *                                jo = floor((x - out_x0) / out_dx + 0.5), io = floor((y - out_y0) / out_dy + 0.5) lies outside
 *                                0 .. out_nx - 1, 0 .. out_ny - 1.
 *     SARX_RELOCATE_OK           the report is kept.
 *     Fields not defined for a status are 0 (rank: -1).
 *     SARX_RELOCATE_OVERFLOW     the input slot has its overflow flag set or count > max_detections: record 0 alone is written,
 *                                every field 0 but the status; the output slot is closed with the input's count and
 *                                overflow = 1.  An overflowing list is an error, never a truncated answer.
 *
 * Output slot: a GMTI slot of max_detections reports that holds the reports of status OK, each copied byte for byte except
 * (i, j) = (io, jo), sorted by (io, jo, r) rising (two reports may share a pixel); count = their number, overflow = 0.
 * Nothing past 64 count_in bytes of the records and nothing past the kept reports of the output slot is touched.
 *
 * Plain C99.  Extends include/sarx.h and include/sarx_gmti.h (the context, the error codes, the slot layout); the limits are
 * those of include/sarx_tdbp_multi.h.
 *
 * Left out: images focused with vel_focus != 0 (the ATI speed is then relative to the focus velocity and the range-rate
 * equation gains a w.vel_focus term), sub-pixel input positions (cluster centroids), moving the pair search's chip, terrain
 * height (the ground is z = 0). */
#ifndef SARX_RELOCATE_H
#define SARX_RELOCATE_H

#include "sarx.h"
#include "sarx_gmti.h"
#include "sarx_tdbp_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_RELOCATE_OK 0u
#define SARX_RELOCATE_NO_SPEED 1u
#define SARX_RELOCATE_NO_SOLUTION 2u
#define SARX_RELOCATE_OFF_GRID 3u
#define SARX_RELOCATE_OVERFLOW 4u

#define SARX_RELOCATE_HAS_VELOCITY 1u  /* flags bit 0 */

typedef struct {
    double pos_ref[3], vel_ref[3]; /* finite */
    double in_x0, in_y0;           /* finite: the image position of pixel (0, 0) */
    double in_dx, in_dy;           /* finite, non-zero: metres per column j, per row i */
    double out_x0, out_y0;         /* finite: the ground position of output pixel (0, 0) */
    double out_dx, out_dy;         /* finite, non-zero */
    int32_t out_nx, out_ny;        /* 1 .. SARX_TDBP_MULTI_MAX_DIM */
    int32_t max_detections;        /* capacity of both slots, 1 .. SARX_TDBP_MULTI_MAX_DETECTIONS */
    int32_t reserved;              /* 0 */
} sarx_relocate_params;            /* 128 bytes */

typedef struct {
    double x, y;                   /* g */
    double shift_x, shift_y;       /* g - q */
    double vx, vy;                 /* ground velocity, valid with flags bit 0 */
    int32_t rank;                  /* index in the output slot, -1 when not kept */
    uint32_t status;               /* SARX_RELOCATE_OK / _NO_SPEED / _NO_SOLUTION / _OFF_GRID / _OVERFLOW */
    uint32_t flags;                /* SARX_RELOCATE_HAS_VELOCITY */
    uint32_t reserved;             /* 0 */
} sarx_relocate_record;            /* 64 bytes */

/* validates the parameters (no device needed): SARX_OK, or SARX_ERR_INVALID and a message naming the field in sarx_last_error(NULL) */
int sarx_relocate_check(const sarx_relocate_params* params);
/* d_slot: the input GMTI slot of max_detections reports (8-byte aligned).  d_v_los: fp64 per report, v_los_stride bytes apart
 * (a multiple of 8, >= 8; 8-byte aligned).  d_valid: uint32 per report, valid_stride bytes apart (a multiple of 4, >= 4; 4-byte
 * aligned), or NULL (its stride is then not looked at).  d_v_along: fp64 per report, v_along_stride apart (as v_los), or NULL.
 * d_records: max_detections sarx_relocate_record; d_out_slot: a GMTI slot of max_detections reports (both 8-byte aligned).  The
 * two outputs may overlap no input (an input array: its first max_detections elements at its stride) and not each other. */
int sarx_relocate_dev(sarx_ctx* ctx, const sarx_relocate_params* params, const void* d_slot, const void* d_v_los, size_t v_los_stride,
                      const void* d_valid, size_t valid_stride, const void* d_v_along, size_t v_along_stride, void* d_records,
                      void* d_out_slot);

#ifdef __cplusplus
}
#endif
#endif /* SARX_RELOCATE_H */
