/* libsarx sliding-window coherence: the complex sample coherence of two complex64 images over a box around every pixel, for ATI
 * phase masking (two channels of one frame) and coherent change detection (two frames of a VideoSAR stack).
 *
 * Plain C99.  Extends include/sarx.h (the context and the error codes come from there).
 *
 * Semantics (device pointers only; a pair call enqueues one launch, two with a summary, on the ctx's current lane; no host
 * synchronisation; nothing is read back):
 *   inputs     : a, b: complex64 [n_az x n_rg] row-major (i = azimuth, j = range), 8-byte aligned, n_az, n_rg >= 1.  a and b may
 *                be the same image; no output may overlap an input or another output
 *   window     : half-widths ha (azimuth), hr (range), each 0 .. SARX_COH_MAX_HALF.  The window of pixel (i, j) is |di| <= ha,
 *                |dj| <= hr clipped to the image; N(i, j) is the number of cells left.  A window larger than the image is allowed
 *   sums       : in fp64, from fp64 products of the fp32 samples (these products are exact):
 *                S12 = sum a conj(b), S11 = sum |a|^2, S22 = sum |b|^2 over the window
 *   coherence  : g = S12 / sqrt(S11 S22) in fp64, g = 0 when S11 S22 = 0
 *                coh (fp32, required)      = |g|, clamped to <= 1
 *                igram (complex64, optional) = g.  The phase is the caller's angle(igram); it is no output of its own because it
 *                is ill-conditioned where |g| is small
 *   change rule: on when a mask or a summary is asked for.  A pixel is TESTED when S11 >= power_floor N and S22 >= power_floor N
 *                (shadow and no-return areas are incoherent in every pair and are no changes); it is CHANGED when it is tested
 *                and the emitted fp32 coh < (float)threshold.
 *                mask (uint8, optional): 0 = not tested, 1 = tested and unchanged, 2 = changed
 *   summary    : optional sarx_coherence_summary, every byte written: n_tested, n_changed, sum_coh = the fp64 sum of the emitted
 *                coh over the tested pixels, n_az, n_rg, reserved words 0.  The order of summation depends on (n_az, n_rg, ha, hr)
 *                alone and no floating-point atomic is used: two calls give the same bytes
 *   stack form : pairs (f, f + lag) of n_frames images frame_stride_bytes apart, lag >= 1, f = 0 .. n_frames - lag - 1; pair f
 *                writes at d_coh + f coh_stride_bytes (igram and mask alike) and summary record f.  The pair launches are
 *                enqueued one behind the other; no host synchronisation
 *
 * The sums run along each direction as running sums that are restarted from a direct sum at the start of every tile (64 rows,
 * 7 columns), never across the image: a sum differs from the direct one by at most (additions) x 2^-53 x the largest power the
 * running sum has held since its restart.  Half-width 0 in a direction takes that direction's sum directly.  Powers are expected to
 * leave S11 S22 finite and normal in fp64.  The workspace holds one partial record per workgroup; its content is not defined. */
#ifndef SARX_COHERENCE_H
#define SARX_COHERENCE_H

#include "sarx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_COH_MAX_HALF 16

typedef struct {
    int32_t ha, hr;                /* half-widths along azimuth and range, 0 .. SARX_COH_MAX_HALF */
    int32_t flags;                 /* 0 (none defined) */
    int32_t reserved;              /* 0 */
    double threshold;              /* finite, >= 0: changed = tested and coh < (float)threshold; 0 = nothing is changed */
    double power_floor;            /* finite, >= 0: tested = S11 >= power_floor N and S22 >= power_floor N */
} sarx_coherence_params;           /* 32 bytes */

typedef struct {
    uint64_t n_tested, n_changed;
    double sum_coh;                /* over the tested pixels */
    uint32_t n_az, n_rg;
    uint32_t reserved[8];          /* 0 */
} sarx_coherence_summary;          /* 64 bytes */

/* validates the parameters for an [n_az x n_rg] image (no device needed) */
int sarx_coherence_check(const sarx_coherence_params* params, int n_az, int n_rg);
/* bytes of the workspace a call with a summary needs for that image (one pair's; the stack form reuses it pair after pair) */
int sarx_coherence_workspace_bytes(const sarx_coherence_params* params, int n_az, int n_rg, size_t* out_bytes);
/* d_coh: fp32 plane (4-byte aligned).  d_igram (complex64, 8-byte aligned), d_mask (uint8) and d_summary (8-byte aligned) may be
 * NULL.  d_workspace (8-byte aligned) is needed with d_summary and may be NULL without it */
int sarx_coherence_pair_dev(sarx_ctx* ctx, const void* d_a, const void* d_b, int n_az, int n_rg, const sarx_coherence_params* params,
                            float* d_coh, void* d_igram, uint8_t* d_mask, void* d_summary, void* d_workspace);
/* the pairs (f, f + lag) of a stack.  Strides are in bytes: frame_stride_bytes >= 8 n_az n_rg and a multiple of 8;
 * coh_stride_bytes >= 4 n_az n_rg and a multiple of 4; igram_stride_bytes >= 8 n_az n_rg and a multiple of 8 (read only with
 * d_igram); mask_stride_bytes >= n_az n_rg (read only with d_mask).  d_summary holds n_frames - lag records */
int sarx_coherence_stack_dev(sarx_ctx* ctx, const void* d_frames, int n_frames, size_t frame_stride_bytes, int lag, int n_az, int n_rg,
                             const sarx_coherence_params* params, float* d_coh, size_t coh_stride_bytes, void* d_igram,
                             size_t igram_stride_bytes, uint8_t* d_mask, size_t mask_stride_bytes, void* d_summary, void* d_workspace);

#ifdef __cplusplus
}
#endif
#endif /* SARX_COHERENCE_H */
