/* libsarx focus-velocity search on the two-receiver back-projection, per GMTI report: for every report of a GMTI slot on the
 * device and every one of n_hyp focus velocities, both receive channels are imaged on a small chip of the pair's ground grid
 * around the report; the DPCA difference of each chip is folded into one record of sharpness figures, the best hypothesis is
 * named per report, and the ATI interferogram is taken at the refocused peak.  The search of
 * sarx_tdbp_search.h sees one channel and therefore the stationary clutter of the chip; the difference of the pair does not.
 *
 * Plain C99.  Extends include/sarx_tdbp_pair.h (the pair's parameter block and pixel arithmetic), include/sarx_tdbp_search.h
 * (the record and its definitions) and include/sarx_gmti.h (the slot: header and report list).
 *
 *    report and chip : report (i, j) addresses pixel row iy = i, column ix = j of the plan's [ny][nx] grid - what gmti_detect on
 *                      a pair produces.  The chip is chip_y rows x chip_x columns at x0 = clamp(j - chip_x / 2, 0, nx - chip_x),
 *                      y0 = clamp(i - chip_y / 2, 0, ny - chip_y): shifted into the grid, never padded.  A report with i or j
 *                      outside the grid gets k_best = -1 in its best record and NOTHING else is written for it.
 *    pixel           : chip (r, h) holds, for both channels, what sarx_tdbp_pair_* gives for vel_focus = vel_hyps[h] at the same
 *                      grid pixels: the same dt (mean over all pulses), float32 interpolation coordinate, pulse ranges,
 *                      chirp_centre_s and fp64 sums in rising pulse order.  The geometry is exact per pixel and pulse, or
 *                      expanded about the reference pixel of each 16 x 16 tile OF THE CHIP when both of the pair's tile
 *                      conditions hold over the whole grid for EVERY hypothesis; sarx_tdbp_pair_search_route tells which ran,
 *                      SARX_TDBP_TILE=0 forces the exact form.
 *    range compression : the plan's, once per channel and call, over one sample window that bounds what any grid pixel can touch
 *                      under every hypothesis (every sample with SARX_TDBP_FULL_RC=1).
 *    record (r, h)   : D = I0 - I1 (SARX_TDBP_PAIR_SEARCH_DPCA) or D = I0 (.._CH0); P = re(D)^2 + im(D)^2 in fp64 (two rounded
 *                      products, one rounded sum); s2 = sum P, s4 = sum P^2 over the chip, peak = max P at (peak_ix, peak_iy) in
 *                      GRID coordinates; of equal maxima the one with the smaller iy * nx + ix.  A NaN power never is the peak;
 *                      if every power is NaN, peak is NaN and the indices are -1.
 *    best (r)        : k_best = argmax over h of s4 (ties: the smaller h; a NaN is never the best unless every s4 is NaN, then 0);
 *                      x0, y0; the peak pixel of k_best; s4 at k_best - 1, k_best, k_best + 1 (-1 past the ends of the list);
 *                      interf = sum of I0 conj(I1) over the 3 x 3 neighbourhood of the peak, clipped to the chip, at k_best (fp64,
 *                      rows then columns rising); p0, p1 = |I0|^2, |I1|^2 at the peak.
 *    slot            : the launches read count and overflow from the device header (no host round trip), process reports
 *                      [0, min(count, max_detections)) and write nothing at all when the slot overflowed (sarx_refocus_dev's
 *                      rule).  The slot itself is only read.
 *    determinism     : pulse chunks summed in chunk order; per record thread t of 256 takes chip pixels t, t + 256, ... in
 *                      rising order, then a binary tree over the 256 threads; no atomics: the same bits from run to run, and
 *                      whether or not the chips are written.
 *    scratch         : belongs to the plan; the first call makes it, a repeated call allocates nothing on the device.  The
 *                      partial sums take max_detections * n_hyp * chunks * 2 * chip_y * chip_x * 16 bytes; the number of pulse
 *                      chunks is chosen from the workgroup count (or is what sarx_tdbp_search_set_chunks set on the plan) and,
 *                      when chosen here, lowered until the partial sums fit SARX_TDBP_PAIR_SEARCH_MAX_PARTIAL_BYTES.  A
 *                      combination that does not fit, or whose max_detections * n_hyp exceeds SARX_TDBP_PAIR_SEARCH_MAX_CHIPS
 *                      (the launch grid's second dimension), is refused with the numbers in the message.
 *
 * Left out: hypotheses per report (a velocity prior per track), relocating the chip by v_los, more than two receivers, and the
 * focus at the estimate enqueued behind the search. */
#ifndef SARX_TDBP_PAIR_SEARCH_H
#define SARX_TDBP_PAIR_SEARCH_H

#include "sarx_gmti.h"
#include "sarx_tdbp_pair.h"
#include "sarx_tdbp_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_TDBP_PAIR_SEARCH_MAX_HYP 64
#define SARX_TDBP_PAIR_SEARCH_MIN_CHIP 4
#define SARX_TDBP_PAIR_SEARCH_MAX_CHIP 64
#define SARX_TDBP_PAIR_SEARCH_MAX_CHIPS 65535                       /* max_detections * n_hyp */
#define SARX_TDBP_PAIR_SEARCH_MAX_PARTIAL_BYTES (256ull << 20)     /* 256 MiB of partial sums */

enum { SARX_TDBP_PAIR_SEARCH_DPCA = 0, SARX_TDBP_PAIR_SEARCH_CH0 = 1 };

typedef struct {
    int32_t chip_x, chip_y;        /* SARX_TDBP_PAIR_SEARCH_MIN_CHIP .. _MAX_CHIP, at most nx and ny; any value, no multiple of 16 needed */
    int32_t n_hyp;                 /* 1 .. SARX_TDBP_PAIR_SEARCH_MAX_HYP */
    int32_t source;                /* SARX_TDBP_PAIR_SEARCH_DPCA or SARX_TDBP_PAIR_SEARCH_CH0 */
} sarx_tdbp_pair_search_params;    /* 16 bytes */

typedef struct {
    int32_t k_best;                /* -1: the report lies outside the grid (nothing else of this record is written) */
    int32_t x0, y0;                /* first column and row of the chip */
    int32_t peak_ix, peak_iy;      /* the peak of D at k_best, grid coordinates */
    int32_t reserved;              /* 0 */
    double s4_prev, s4_best, s4_next;   /* s4 at k_best - 1, k_best, k_best + 1; -1 past the ends */
    double interf_re, interf_im;   /* sum I0 conj(I1) over the clipped 3 x 3 neighbourhood of the peak, at k_best */
    double p0, p1;                 /* |I0|^2, |I1|^2 at the peak */
} sarx_tdbp_pair_search_best;      /* 80 bytes */

/* params alone, against a grid when nx, ny > 0 (0: not known yet): SARX_OK, or SARX_ERR_INVALID and a message in
 * sarx_last_error(NULL).  Needs no device. */
int sarx_tdbp_pair_search_check(const sarx_tdbp_pair_search_params* params, int nx, int ny);
/* d_raw0, d_raw1, pos_tx, vel_tx, t_pulses, t_start, scene_size, pair: as sarx_tdbp_pair_dev takes them.  vel_hyps [n_hyp][3]: host
 * fp64, finite, shared by all reports.  d_reports, d_header: the device slot (8- and 4-byte aligned), max_detections >= 1 its
 * capacity.  d_records: device [max_detections][n_hyp] (8-byte aligned); d_best: device [max_detections] (8-byte aligned);
 * d_chips: device complex128 [max_detections][n_hyp][2][chip_y][chip_x] (16-byte aligned) or NULL = not written.  Returns after
 * the small uploads are enqueued; everything runs on the ctx's current lane. */
int sarx_tdbp_pair_search_dev(sarx_tdbp_plan* plan, const void* d_raw0, const void* d_raw1, const double* pos_tx, const double* vel_tx,
                              const double* t_pulses, double t_start, double scene_size, const sarx_tdbp_pair_params* pair,
                              const double* vel_hyps, const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header,
                              int max_detections, const sarx_tdbp_pair_search_params* params, sarx_tdbp_search_record* d_records,
                              sarx_tdbp_pair_search_best* d_best, void* d_chips);
/* blocking; raw0, raw1, reports, header, records, best and chips (or NULL) are host memory.  Of the outputs only what the device
 * form writes is touched. */
int sarx_tdbp_pair_search_host(sarx_tdbp_plan* plan, const void* raw0, const void* raw1, const double* pos_tx, const double* vel_tx,
                               const double* t_pulses, double t_start, double scene_size, const sarx_tdbp_pair_params* pair,
                               const double* vel_hyps, const sarx_gmti_report* reports, const sarx_gmti_header* header,
                               int max_detections, const sarx_tdbp_pair_search_params* params, sarx_tdbp_search_record* records,
                               sarx_tdbp_pair_search_best* best, void* chips);
/* *tile = 1 when the plan's last pair search took the tile-expanded kernel, 0 for the exact one; SARX_ERR_INVALID before any */
int sarx_tdbp_pair_search_route(const sarx_tdbp_plan* plan, int* tile);

#ifdef __cplusplus
}
#endif
#endif /* SARX_TDBP_PAIR_SEARCH_H */
