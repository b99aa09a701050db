/* libsarx phase-gradient autofocus (PGA): a non-parametric azimuth phase error estimated from an image's own bright points and
 * removed, for one frame or a stack of frames.
 *
 * Plain C99.  Extends include/sarx.h (the context and the error codes come from there).
 *
 * Data: complex64 images, n_frames >= 1 of them; frame f starts at d_in + f frame_stride (in elements), element (i, j) lies at
 *   i ld + j (i = azimuth, j = range), n_az = L in {64, 128, 256, 512, 1024}, n_rg >= 1, ld >= n_rg (a strip or a chip of a
 *   larger image is addressed in place).  d_out has the layout of d_in and must not overlap it.  Columns n_rg .. ld - 1 of d_out
 *   are not written.
 *
 * Semantics.  k indexes azimuth frequency in fftshift order: bin u = (k - L/2) mod L of the L-point FFT along i.  phi_tot[k]
 * starts at 0, g_0 is the input and g_it = ifft(fft(g_0) exp(-j phi_tot)) after `it` updates (1/L on the inverse): the apply step
 * always transforms the input, so rounding does not accumulate over the iterations.
 *
 * Estimate `it`, on g_it, per frame:
 *   1. per column j: p = |g|^2 (fp32); peak row r_j = argmax_i p (ties: the smaller i); contrast c_j = p[r_j] / mean_i p (the
 *      mean from an fp64 sum); the column is used when p[r_j] > 0 and c_j >= min_contrast
 *   2. a used column is rotated circularly so that r_j comes to row 0, rows whose circular distance from 0 exceeds
 *      half_width[it] are zeroed, and the result is transformed: G_j[k]
 *   3. over the used columns, fp64, in a fixed order: P[k] = sum_j |G_j[k]|^2, S[k] = sum_j G_j[k] conj(G_j[k-1]) (k >= 1)
 *   4. bin k is supported when P[k] > power_floor max_k P;  D[k] = arg S[k] when k >= 1 and both k and k - 1 are supported,
 *      else 0;  phi[k] = sum_{m <= k} D[m]
 *   5. over the supported bins the least-squares line (mean and slope, unit weights, fp64) is subtracted; unsupported bins get
 *      0; with fewer than two supported bins phi = 0
 *   6. the record: s2 = sum |g_it|^2, s4 = sum |g_it|^4 over the frame (fp32 products, fp64 sums), rms_phase = rms of phi over
 *      the supported bins, n_cols_used, n_bins_supported
 * Update: phi_tot += phi, for it < n_iter.  The estimate runs once more on g_{n_iter} = d_out: record n_iter; its phi is the
 * residual and is not applied, its rms_phase is the convergence figure.
 *
 * Outputs: d_out;  d_phase [n_frames x L] fp64 = phi_tot;  d_records [n_frames x (n_iter + 1)].  Every sum is a fixed tree or a
 * fixed-order second stage, there are no atomics: frame f of a stack gives the bits of that frame alone, two runs give the same
 * bits. */
#ifndef SARX_PGA_H
#define SARX_PGA_H

#include "sarx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_PGA_MAX_ITER 8        /* iterations per call */
#define SARX_PGA_MAX_RG (1 << 20)  /* columns of a frame */
#define SARX_PGA_MAX_FRAMES 65535  /* frames per call */

typedef struct {
    int32_t n_iter;                            /* 1 .. SARX_PGA_MAX_ITER */
    int32_t half_width[SARX_PGA_MAX_ITER];     /* h_it >= 1 with 2 h_it + 1 <= L, it < n_iter; the final estimate uses h_{n_iter - 1} */
    int32_t reserved;                          /* 0 */
    double min_contrast;                       /* >= 0 */
    double power_floor;                        /* in [0, 1) */
} sarx_pga_params;                             /* 56 bytes */

typedef struct {
    double s2, s4;                             /* sum |g_it|^2, sum |g_it|^4 over the frame */
    double rms_phase;                          /* rms of this estimate's phi over the supported bins (rad) */
    int32_t n_cols_used;
    int32_t n_bins_supported;
} sarx_pga_record;                             /* 32 bytes */

/* validates the parameters and the layout (no device needed); frame_stride is not looked at when n_frames == 1 */
int sarx_pga_check(const sarx_pga_params* params, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride);
/* bytes of the workspace sarx_pga_dev needs for this layout (the tiles' partial sums; its content is not defined afterwards) */
int sarx_pga_workspace_bytes(const sarx_pga_params* params, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride,
                             size_t* out_bytes);
/* all n_iter + 1 estimates and n_iter applies on the ctx's current lane: device pointers only, no host synchronisation */
int sarx_pga_dev(sarx_ctx* ctx, const void* d_in, void* d_out, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride,
                 const sarx_pga_params* params, double* d_phase, sarx_pga_record* d_records, void* d_workspace);
/* the apply step alone: out = ifft(fft(in) exp(j sign phase)), sign = -1 corrects, +1 injects.  Frame f takes the L phases at
 * d_phase + f phase_stride (in elements; 0 = one phase for every frame, else >= L); d_phase is not written */
int sarx_pga_apply_dev(sarx_ctx* ctx, const void* d_in, void* d_out, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride,
                       const double* d_phase, size_t phase_stride, int sign);

#ifdef __cplusplus
}
#endif
#endif /* SARX_PGA_H */
