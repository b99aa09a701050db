/* libsarx GMTI detection: CA-CFAR on the DPCA magnitude plane, refined with the ATI interferogram.
 *
 * Plain C99.  Extends include/sarx.h (contexts, buffers, error codes and sarx_last_error come from there).
 *
 * Semantics (both launches run on the ctx's current lane, device pointers only, no host synchronisation):
 *   m[i, j]   : the DPCA magnitude plane, [n_az x n_rg] row-major fp32 (i = azimuth, j = range)
 *   P         = (double)m * (double)m
 *   guard box : |di| <= guard_az, |dj| <= guard_rg (holds the cell under test)
 *   outer box : |di| <= guard_az + train_az, |dj| <= guard_rg + train_rg
 *   T(i, j)   : cells of the outer box inside the image, minus the guard box;  N = |T|
 *   a cell is tested when N >= min_train, detected when P > alpha * mean_T(P) (sums and mean in fp64; edge cells keep the
 *   caller's alpha), and REPORTED when it is detected and its P is the maximum over its guard box (ties: the smaller linear
 *   index i * n_rg + j wins).  guard + train <= SARX_GMTI_MAX_HALF in both directions.
 *
 * Output slot = one sarx_gmti_header followed by max_detections sarx_gmti_report (sarx_gmti_slot_bytes).  After
 * sarx_gmti_cfar_dev + sarx_gmti_refine_dev the header holds the number of qualifying cells and the reports
 * [0, min(count, max_detections)) are sorted by (i, j) and complete.  count > max_detections sets `overflow`: which cells made
 * it into the list is then not defined, and callers must treat the slot as an error, never as a truncated answer. */
#ifndef SARX_GMTI_H
#define SARX_GMTI_H

#include "sarx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_GMTI_MAX_HALF 32      /* guard + train half-width limit per direction (the CFAR tile's halo) */

typedef struct {
    int32_t guard_az, guard_rg;    /* guard half-widths (>= 0) */
    int32_t train_az, train_rg;    /* training half-widths (>= 0; the training set must not be empty) */
    double alpha;                  /* threshold factor (> 0); for exponential power alpha = N_full (pfa^(-1/N_full) - 1) */
    int32_t min_train;             /* a cell is tested only with at least this many training cells (>= 1) */
    int32_t max_detections;        /* capacity of the report list (>= 1) */
} sarx_gmti_params;

typedef struct {
    uint32_t count;                /* qualifying cells found (may exceed max_detections) */
    uint32_t overflow;             /* 1 when count > max_detections */
    uint32_t reserved[2];
} sarx_gmti_header;                /* 16 bytes */

typedef struct {
    int32_t i, j;                  /* azimuth row, range column */
    double power;                  /* P of the cell */
    double mean;                   /* mean_T(P) */
    double interf_re, interf_im;   /* sum over the 3 x 3 neighbourhood (clipped) of slc1 conj(slc2 e^{j cal_phase}), fp64 */
    float mag1, mag2;              /* |slc1|, |slc2| at the cell */
} sarx_gmti_report;                /* 48 bytes */

/* bytes of one output slot for these parameters (header + max_detections reports); validates the parameters */
int sarx_gmti_slot_bytes(const sarx_gmti_params* params, size_t* out_bytes);
/* CFAR launch: zeroes the header, then appends (i, j, power, mean) of every reported cell (order not defined yet) */
int sarx_gmti_cfar_dev(sarx_ctx* ctx, const float* d_dpca_mag, int n_az, int n_rg, const sarx_gmti_params* params,
                       sarx_gmti_report* d_reports, sarx_gmti_header* d_header);
/* refine launch: reads the count from the device header (no host round trip), sorts the first min(count, max_detections)
 * reports by (i, j) and fills interf / mag1 / mag2 from the complex64 images [n_az x n_rg] */
int sarx_gmti_refine_dev(sarx_ctx* ctx, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, double cal_phase,
                         sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_detections);

#ifdef __cplusplus
}
#endif
#endif /* SARX_GMTI_H */
