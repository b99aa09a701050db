/* libsarx GMTI detection, ordered-statistic CFAR (OS-CFAR, Rohling) on the DPCA magnitude plane.
 *
 * Plain C99.  Extends include/sarx_gmti.h: the launch below stands where sarx_gmti_cfar_dev stands and writes the same slot
 * (sarx_gmti_header + sarx_gmti_report[]), so sarx_gmti_refine_dev, sarx_refocus_dev and the tracker take its result unchanged.
 *
 * Taken from sarx_gmti.h unchanged: m and P = (double)m * (double)m (exact); the guard box, the outer box and the training set
 * T(i, j) = the outer box clipped to the image minus the guard box, N = |T| (cells outside the image are not in T: they do not
 * count as zeros); N_full = N of a window wholly inside the image; guard + train <= SARX_GMTI_MAX_HALF per direction; the peak
 * rule and its tie rule; max_detections, count, overflow and the slot layout.  m >= 0 (a magnitude).
 *
 * New:
 *   rank      : 1 <= rank <= N_full
 *   k         = (rank * N + N_full - 1) / N_full in integers: the rank scaled to the cell's N, rounded up, >= 1, = rank where
 *               the window lies inside the image
 *   a cell is tested when N >= min_train, and DETECTED when P > 0 and
 *                 #{ t in T : alpha * P_t < P }  >=  k
 *               with alpha * P_t one IEEE fp64 product of alpha and the exact P_t, and a strict comparison.  Rounding is
 *               monotone, so this is exactly P > alpha * x_(k) with x_(k) the k-th smallest P_t of T; the count is what the
 *               device evaluates.  Edge cells (N < N_full) keep the caller's alpha.
 *   a cell is REPORTED when it is detected and is the peak of its guard box (sarx_gmti.h).
 *   A reported cell's `mean` field holds x_(k) itself in fp64: the clutter level the cell was held against.
 * After sarx_gmti_oscfar_dev + sarx_gmti_refine_dev the reports are sorted by (i, j) and complete. */
#ifndef SARX_OSCFAR_H
#define SARX_OSCFAR_H

#include "sarx_gmti.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    sarx_gmti_params base;         /* half-widths, alpha (for exponential power: the root of
                                      prod_{i < rank} (N_full - i) / (N_full - i + alpha) = pfa), min_train, max_detections */
    int32_t rank;                  /* 1 .. N_full */
    int32_t flags;                 /* 0: none is defined */
} sarx_oscfar_params;              /* 40 bytes */

/* SARX_OK when the launch would accept these parameters, else the code it would return (message: sarx_last_error(NULL)) */
int sarx_oscfar_check(const sarx_oscfar_params* params);
/* OS-CFAR launch on the ctx's current lane: zeroes the header, then appends (i, j, power, level) of every reported cell (order
 * not defined until sarx_gmti_refine_dev).  Device pointers, [n_az x n_rg] row-major fp32; no host synchronisation.  Every
 * refusal (those of sarx_gmti_cfar_dev, rank outside 1 .. N_full, flags != 0) is made before anything is enqueued. */
int sarx_gmti_oscfar_dev(sarx_ctx* ctx, const float* d_dpca_mag, int n_az, int n_rg, const sarx_oscfar_params* params,
                         sarx_gmti_report* d_reports, sarx_gmti_header* d_header);

#ifdef __cplusplus
}
#endif
#endif /* SARX_OSCFAR_H */
