/* libsarx GMTI ATI gate: the second step of the two-step DPCA / ATI detector, on the device.  A report is kept only when its
 * interferometric phase stands out from the phase of the clutter around it; the margin follows from the clutter's coherence and
 * the number of looks.  The residue of a bright stationary scatterer after an imperfect channel balance passes the CFAR on the
 * DPCA magnitude but carries the clutter's phase, and goes here.
 *
 * Plain C99.  Extends include/sarx.h and include/sarx_gmti.h (the context, the error codes and the slot layout come from there).
 *
 * Input: a GMTI slot, one sarx_gmti_header followed by max_detections sarx_gmti_report exactly as sarx_gmti_refine_dev leaves it
 * (count n read from the device header: no entry point synchronises with the host), and the complex64 images a = slc1, b = slc2,
 * [n_az x n_rg] row-major (i = azimuth, j = range), 8-byte aligned.  Only i and j of a report are read; the rest is copied.
 *
 * Output: a slot of the same layout that holds the kept reports (sorted by (i, j) like the input, so sarx_cluster_step_dev,
 * sarx_refocus_dev, sarx_track_step_dev and every decoder of a GMTI slot take it unchanged) and, when asked for, one
 * sarx_atigate_stat per input report.
 *
 *    0. overflow     : the input header's overflow flag set or count > max_detections: the output header becomes
 *                      {count, 1, 0, 0}, nothing else is written (no statistics either).  A truncated list is never gated.
 *    per report r at (i, j), boxes as in sarx_gmti.h: guard box |di| <= guard_az, |dj| <= guard_rg; outer box
 *    |di| <= guard_az + train_az, |dj| <= guard_rg + train_rg; look box |di| <= look_az, |dj| <= look_rg (inside the guard box):
 *    1. ring T       : the cells of the outer box inside the image, minus the guard box;  N = |T|.
 *                      c11 = sum_T |a|^2,  c22 = sum_T |b|^2,  c12 = sum_T a conj(b).  Every term is the exact fp64 product of two
 *                      fp32 samples (re re, im im, ...: two terms per cell and component), the sums are fp64.  The ring's cells are
 *                      summed themselves, never as outer box minus guard box: a target 60 dB over the clutter in the guard box
 *                      would leave its rounding error in the difference.
 *    2. look box L   : clipped to the image, n_look = |L|;  I = sum_L a conj(b), summed the same way.
 *    3. untested     : N < min_train (reason 1);  else c11 c22 == 0 (the fp64 product) or I == 0 (reason 2);  else with
 *                      den = sqrt(c11 c22), g = c12 / den, coh = min(|g|, 1) (|g| = hypot): coh < min_coh (reason 3).
 *                      A report whose (i, j) lies outside the image has N = n_look = 0 and all sums 0: reason 1.
 *    4. otherwise    : psi = atan2(im, re) of I conj(c12) (re = I_re c12_re + I_im c12_im, im = I_im c12_re - I_re c12_im): the
 *                      report's phase against the local clutter phase, so cal_phase and any slow phase ramp cancel;
 *                      sigma = sqrt((1 - coh^2) / (2 n_look coh^2)), the Cramer-Rao spread of an n_look-look interferogram of
 *                      that coherence (+inf for coh == 0, which only min_coh == 0 lets through).
 *    5. decision     : thr = k_sigma * sigma, one rounded product.  PASSED when fabs(psi) > thr && fabs(psi) >= phase_min, else
 *                      REJECTED (so also when thr is NaN).
 *    6. kept         : a report that passed, or that is untested while SARX_ATIGATE_KEEP_UNTESTED is set.
 *    7. output slot  : header {n_kept, 0, 0, 0}; the kept reports, byte-for-byte copies in rising input index.  Nothing past
 *                      16 + 48 n_kept bytes is touched.
 *    8. statistics   : stats[r] for r < n, nothing past 96 n bytes.  The six sums, n_train = N and n_look always; coh from
 *                      reason 3 on, psi and sigma for tested reports, 0 where they are not defined; status 0 untested, 1 rejected,
 *                      2 passed; reason 0 unless untested; out_index = the report's place in the output slot, -1 when dropped.
 *    9. consequences : n_kept <= n, so the stage never overflows.  With k_sigma = 0, phase_min = 0 and KEEP_UNTESTED the first
 *                      16 + 48 n bytes of the output slot equal the input's (a header whose reserved words are 0), but for a
 *                      tested report whose psi is exactly 0 (`>`; the two images identical, say).  Every output is the same bytes
 *                      from run to run: the reduction order is fixed, there are no floating-point and no global atomics.
 *                      NaN or Inf samples give NaN sums and an unspecified decision, never an access outside the buffers.
 *
 * Left out: a threshold from the exact multilook phase distribution instead of the Cramer-Rao spread, reuse of a full-plane
 * coherence map (sarx_coherence.h) where a caller already has one, a global phase reference for scenes without clutter (their
 * reports are untested, and kept with KEEP_UNTESTED), and gating in relocated ground coordinates. */
#ifndef SARX_ATIGATE_H
#define SARX_ATIGATE_H

#include "sarx.h"
#include "sarx_gmti.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_ATIGATE_MAX_LOOK 4
#define SARX_ATIGATE_MAX_DETECTIONS 16384
#define SARX_ATIGATE_MAX_DIM (1 << 30)     /* n_az and n_rg */
#define SARX_ATIGATE_KEEP_UNTESTED 1u      /* flags bit 0 */

#define SARX_ATIGATE_UNTESTED 0
#define SARX_ATIGATE_REJECTED 1
#define SARX_ATIGATE_PASSED 2
#define SARX_ATIGATE_REASON_TRAIN 1        /* N < min_train */
#define SARX_ATIGATE_REASON_ZERO 2         /* c11 c22 == 0 or I == 0 */
#define SARX_ATIGATE_REASON_COHERENCE 3    /* coh < min_coh */

typedef struct {
    int32_t guard_az, guard_rg;    /* guard half-widths (>= 0) */
    int32_t train_az, train_rg;    /* training half-widths (>= 0; guard + train <= SARX_GMTI_MAX_HALF; the ring must not be empty) */
    int32_t look_az, look_rg;      /* look half-widths, 0 .. SARX_ATIGATE_MAX_LOOK and <= guard_az, guard_rg */
    double k_sigma;                /* threshold in Cramer-Rao spreads (finite, >= 0) */
    double phase_min;              /* least |psi| of a mover, radians, 0 .. pi */
    double min_coh;                /* clutter coherence below which a report is untested, 0 .. 1 */
    int32_t min_train;             /* a report is tested only with at least this many ring cells (>= 1) */
    int32_t max_detections;        /* capacity of both slots, 1 .. SARX_ATIGATE_MAX_DETECTIONS */
    uint32_t flags;                /* SARX_ATIGATE_KEEP_UNTESTED; every other bit 0 */
    uint32_t reserved;             /* 0 */
} sarx_atigate_params;             /* 64 bytes */

typedef struct {
    double c11, c22;               /* ring sums of |a|^2 and |b|^2 */
    double c12_re, c12_im;         /* ring sum of a conj(b) */
    double i_re, i_im;             /* look-box sum of a conj(b) */
    double coh, psi, sigma;
    int32_t n_train, n_look;
    int32_t status;                /* SARX_ATIGATE_UNTESTED / _REJECTED / _PASSED */
    int32_t reason;                /* SARX_ATIGATE_REASON_* when untested, else 0 */
    int32_t out_index;             /* place in the output slot, -1 when dropped */
    int32_t reserved;              /* 0 */
} sarx_atigate_stat;               /* 96 bytes */

/* validates the parameters (no device needed) */
int sarx_atigate_check(const sarx_atigate_params* params);
/* bytes of the statistics of one frame (max_detections sarx_atigate_stat) */
int sarx_atigate_stats_bytes(const sarx_atigate_params* params, size_t* out_bytes);
/* one frame: the slot at d_slot_in into the slot at d_slot_out (both 8-byte aligned, sarx_gmti_slot_bytes long), against the images
 * d_slc1, d_slc2 (8-byte aligned, n_az and n_rg 1 .. SARX_ATIGATE_MAX_DIM).  d_stats: max_detections sarx_atigate_stat (8-byte
 * aligned) or NULL.  Neither output may overlap an input or the other output: SARX_ERR_INVALID.  Two launches on the ctx's current
 * lane (the sums and decisions, one workgroup per report; the compaction, one workgroup), only enqueued. */
int sarx_atigate_step_dev(sarx_ctx* ctx, const sarx_atigate_params* params, const void* d_slc1, const void* d_slc2, int n_az, int n_rg,
                          const void* d_slot_in, void* d_slot_out, void* d_stats);

#ifdef __cplusplus
}
#endif
#endif /* SARX_ATIGATE_H */
