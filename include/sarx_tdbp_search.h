/* libsarx focus-velocity search of the time-domain back-projection: the image of one CPI under many focus velocities in one
 * enqueue, and per velocity one small record of sharpness figures.  The VideoSAR path's sarx_tdbp_focus_* needs the target's
 * velocity; a line search over these records estimates its along-track component from the data.
 *
 * Plain C99.  Extends include/sarx.h: the context, the error codes, sarx_tdbp_plan and the argument conventions of
 * sarx_tdbp_focus_dev / _host come from there.
 *
 *    per call       : the pulses are range-compressed ONCE, over the union of the sample windows of all hypotheses (each the
 *                     geometric bound of sarx_tdbp_focus_*, so still a bound); one per-pulse table and one hypothesis table
 *                     [n_hyp][3] are uploaded.
 *    per hypothesis : the image I_h [ny][nx] complex128 that sarx_tdbp_focus_* gives for vel_focus = vel_hyps[h] (the same
 *                     arithmetic, float32 interpolation coordinate, pulse order per pixel and fp64 accumulation; the
 *                     tile-expanded kernel when its condition holds for EVERY hypothesis, else the exact one), and
 *                     P = re^2 + im^2 (fp64: two rounded products, one rounded sum),
 *                     s2 = sum P,  s4 = sum P^2,  peak = max P at (peak_ix, peak_iy); of equal maxima the one with the
 *                     smaller iy * nx + ix.  A NaN power never is the peak; if every power is NaN, peak is NaN and the
 *                     indices are -1.
 *    determinism    : the sums run in a fixed order (pixels t, t + 1024, ... per thread, then a binary tree over 1024 threads),
 *                     no atomics: records are the same bits from run to run, and whether or not the stack is written.
 *    scratch        : belongs to the plan; it grows on the first call of a given n_hyp, a repeated call allocates nothing on the
 *                     device.  As with sarx_tdbp_focus_dev, a plan serves one lane at a time.
 *
 * The radial (ground-range) velocity component is not estimated here (a mismatch there displaces the target instead of defocusing
 * it): it is measured from the second receive channel, include/sarx_tdbp_pair.h.
 * Left out: normalising the sums when the target leaves the chip, a search per tracker report, and taking the estimate
 * without a host read of the records. */
#ifndef SARX_TDBP_SEARCH_H
#define SARX_TDBP_SEARCH_H

#include "sarx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_TDBP_SEARCH_MAX_HYP 1024
#define SARX_TDBP_SEARCH_MAX_CHUNKS 64

typedef struct {
    double s2, s4, peak;
    int32_t peak_ix, peak_iy;
} sarx_tdbp_search_record;         /* 32 bytes */

/* d_raw: device complex64 [n_pulses][num_samples]; pos, vel [n_pulses][3], t_pulses [n_pulses], vel_hyps [n_hyp][3]: host fp64,
 * every velocity finite, 1 <= n_hyp <= SARX_TDBP_SEARCH_MAX_HYP.  d_images: device complex128 [n_hyp][ny][nx] or NULL;
 * d_records: device [n_hyp].  Returns after the two small uploads are enqueued; everything runs on the ctx's current lane. */
int sarx_tdbp_search_dev(sarx_tdbp_plan* plan, const void* d_raw, const double* pos, const double* vel, const double* t_pulses,
                         double t_start, const double* vel_hyps, int n_hyp, double scene_size, void* d_images,
                         sarx_tdbp_search_record* d_records);
/* blocking; raw, images (or NULL) and records are host memory */
int sarx_tdbp_search_host(sarx_tdbp_plan* plan, const void* raw, const double* pos, const double* vel, const double* t_pulses,
                          double t_start, const double* vel_hyps, int n_hyp, double scene_size, void* images,
                          sarx_tdbp_search_record* records);
/* *tile = 1 when the plan's last search took the tile-expanded kernel, 0 for the exact one; SARX_ERR_INVALID before any search */
int sarx_tdbp_search_route(const sarx_tdbp_plan* plan, int* tile);
/* pulse chunks of the plan's later searches: 1 .. SARX_TDBP_SEARCH_MAX_CHUNKS, or 0 (the default) = chosen from the grid size.
 * The chunk sums are added in chunk order, so the last bits of an image may depend on this number (the terms are fp32 values
 * added in fp64: as long as every partial sum is exact they do not). */
int sarx_tdbp_search_set_chunks(sarx_tdbp_plan* plan, int chunks);
/* the metric launch alone: records of a device stack [n_hyp][ny][nx] complex128 the caller holds (nothing else is read) */
int sarx_tdbp_search_metric_dev(sarx_tdbp_plan* plan, const void* d_stack, int n_hyp, sarx_tdbp_search_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* SARX_TDBP_SEARCH_H */
