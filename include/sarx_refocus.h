/* libsarx GMTI refocus: an azimuth FM-rate search on a chip around each GMTI report.
 *
 * Plain C99.  Extends include/sarx_gmti.h (the report list and its header come from there).
 *
 * Semantics (one call enqueues two launches on the ctx's current lane, device pointers only, no host synchronisation):
 *   images    : complex64 slc1, slc2 [n_az x n_rg] row-major (i = azimuth, j = range)
 *   source    : SARX_REFOCUS_DPCA: x = slc1 - slc2 e^{j cal_phase};  SARX_REFOCUS_SLC1: x = slc1 (slc2 may be NULL)
 *   chip      : L rows x W columns around report (i, j); rows i0 .. i0 + L - 1 with i0 = clamp(i - L/2, 0, n_az - L) (shifted into
 *               the image, never padded), columns j - W/2 .. j + W/2 (zero outside the image).  L in {64, 128, 256, 512},
 *               L <= n_az; W odd, 1 .. SARX_REFOCUS_MAX_W
 *   filter    : Y_k = ifft_az(fft_az(x) H_k) (1/L on the inverse), H_k(f, c) = exp(j 4 pi R_c / lambda (D(f; V'_k) - D(f; V_r))),
 *               f = fftfreq(L, 1/prf), D(f; V) = sqrt(1 - (lambda f / 2V)^2) (negative arguments clamped to 1e-9),
 *               R_c = r0 + j_c dr the range of column j_c.  The phase is formed as (lambda f / 2)^2 (1/V_r^2 - 1/V'^2) / (D' + D)
 *               in fp64 and reduced to revolutions before an fp32 sincos; V'_k = V_r leaves the chip unchanged.
 *   metric    : S_k = sum |Y_k|^4 / (sum |x|^2)^2 over the chip (fp32 products, fp64 sums in a fixed order);
 *               k* = argmax S_k (ties: the smaller k);  S_id = the same metric of x itself
 *
 * The launches read count and overflow from the GMTI header (no host round trip), process reports [0, min(count,
 * max_detections)) and write nothing at all when the slot overflowed.  Record r belongs to report r.  Optional outputs (NULL =
 * not written): curves [max_detections x n_hyp] fp32 S_k;  chips [max_detections x L x W] complex64 Y_{k*}, row-major. */
#ifndef SARX_REFOCUS_H
#define SARX_REFOCUS_H

#include "sarx_gmti.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_REFOCUS_MAX_HYP 64    /* hypotheses per call */
#define SARX_REFOCUS_MAX_W 15      /* chip width in range cells (odd) */

enum { SARX_REFOCUS_DPCA = 0, SARX_REFOCUS_SLC1 = 1 };

typedef struct {
    int32_t chip_az;               /* L: 64, 128, 256 or 512 */
    int32_t chip_rg;               /* W: odd, 1 .. SARX_REFOCUS_MAX_W */
    int32_t source;                /* SARX_REFOCUS_DPCA or SARX_REFOCUS_SLC1 */
    int32_t n_hyp;                 /* 1 .. SARX_REFOCUS_MAX_HYP */
    double wavelength_m;           /* lambda (> 0) */
    double platform_speed_mps;     /* V_r of the focuser's azimuth filter (> 0) */
    double prf_hz;                 /* > 0 */
    double r0_m, dr_m;             /* range of column j: r0 + j dr (the focuser's axis) */
    double cal_phase;              /* channel balance of the DPCA source (rad) */
    double speed_mps[SARX_REFOCUS_MAX_HYP];   /* V'_k, k < n_hyp (> 0) */
} sarx_refocus_params;             /* 576 bytes */

typedef struct {
    int32_t k_best;                /* k* */
    int32_t i0;                    /* first chip row */
    int32_t peak_i, peak_j;        /* argmax |Y_{k*}|^2 over the chip's in-image cells, image coordinates (ties: smaller index) */
    float s_prev, s_best, s_next;  /* S_{k*-1}, S_{k*}, S_{k*+1}; -1 past the ends of the grid */
    float s_identity;              /* S_id */
    float peak_power;              /* |Y_{k*}|^2 at the peak */
    float orig_power;              /* max |x|^2 over the chip */
    int32_t reserved[2];
} sarx_refocus_record;             /* 48 bytes */

/* validates the parameters for an [n_az x n_rg] image (no device needed) */
int sarx_refocus_check(const sarx_refocus_params* params, int n_az, int n_rg);
/* both launches on the ctx's current lane: a record per report into d_records [max_detections], and the optional curves / chips */
int sarx_refocus_dev(sarx_ctx* ctx, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, const sarx_refocus_params* params,
                     const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_detections,
                     sarx_refocus_record* d_records, float* d_curves, void* d_chips);

#ifdef __cplusplus
}
#endif
#endif /* SARX_REFOCUS_H */
