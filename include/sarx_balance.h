/* libsarx two-channel balance: a block-adaptive complex weight for channel 2 and a coherence value per block.
 *
 * Plain C99.  Extends include/sarx.h (the context and the error codes come from there).
 *
 * Semantics (device pointers only; estimate enqueues two launches and apply one on the ctx's current lane, no host
 * synchronisation; nothing is read back):
 *   images    : complex64 slc1, slc2 [n_az x n_rg] row-major (i = azimuth, j = range), 8-byte aligned
 *   blocks    : block_az x block_rg pixels, each SARX_BALANCE_MIN_BLOCK .. SARX_BALANCE_MAX_BLOCK; nb_az = ceil(n_az / block_az),
 *               nb_rg = ceil(n_rg / block_rg), nb_az nb_rg <= SARX_BALANCE_MAX_BLOCKS.  The last block in each direction is
 *               ragged; a block larger than the image gives one block.  Block b = ba nb_rg + br.
 *   kept      : a pixel is kept when |s1|^2 <= clip and |s2|^2 <= clip, both formed in fp32 as fmaf(re, re, im * im) (im * im
 *               rounded to fp32 first) and compared with clip = min((float)clip_power, FLT_MAX): clip_power = +inf keeps every
 *               pixel whose fp32 power is finite
 *   sums      : per block over its kept pixels, products and sums in fp64 (the fp64 products of fp32 samples are exact):
 *               S12 = sum s1 conj(s2), S11 = sum |s1|^2, S22 = sum |s2|^2, n = pixels kept.  The order of summation depends on
 *               (n_az, n_rg, block_az, block_rg) alone - not on the grid, the device, the buffers' addresses or timing - and no
 *               floating-point atomic is used: two calls give the same bits.
 *   weight    : SARX_BALANCE_LS: w = S12 / S22 (minimises sum |s1 - w s2|^2);  SARX_BALANCE_PHASE: w = S12 / |S12|
 *   coherence : gamma = |S12| / sqrt(S11 S22) (0 when S11 S22 = 0)
 *   valid     : n >= min_count, S22 > 0, |S12| > 0 and gamma >= min_coherence
 *   global    : weight and coherence by the same formulas from the sums of S12, S11, S22 over the valid blocks; invalid blocks
 *               take the global weight.  No valid block (or a vanishing global |S12|): global weight 1 + 0j, n_valid = 0
 *               tells the caller.
 *   per pixel : SARX_BALANCE_NEAREST: the weight of the pixel's own block.  SARX_BALANCE_BILINEAR: re and im interpolated
 *               separately over the nominal block centres (ragged blocks keep their nominal centre), per direction
 *               t = clamp((i + 0.5) / block - 0.5, 0, nb - 1), b0 = min(floor(t), max(nb - 2, 0)), f = t - b0,
 *               b1 = min(b0 + 1, nb - 1): constant outside the outermost centres.  Interpolation and the complex multiply run
 *               in fp32.
 *   outputs   : slc2_out = w(i, j) slc2 (complex64; may be slc2 itself);  optional dpca_mag = |slc1 - slc2_out| (fp32, hypotf)
 *
 * The table is a sarx_balance_header followed by nb_az nb_rg sarx_balance_record; every byte of it is written by every
 * estimate call (reserved words as 0).  The workspace holds the partial sums of the strips a block is cut into; its content
 * is not defined. */
#ifndef SARX_BALANCE_H
#define SARX_BALANCE_H

#include "sarx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_BALANCE_MIN_BLOCK 8
#define SARX_BALANCE_MAX_BLOCK 4096
#define SARX_BALANCE_MAX_BLOCKS 65536

enum { SARX_BALANCE_LS = 0, SARX_BALANCE_PHASE = 1 };
enum { SARX_BALANCE_NEAREST = 0, SARX_BALANCE_BILINEAR = 1 };

typedef struct {
    int32_t block_az, block_rg;    /* SARX_BALANCE_MIN_BLOCK .. SARX_BALANCE_MAX_BLOCK */
    int32_t mode;                  /* SARX_BALANCE_LS or SARX_BALANCE_PHASE */
    int32_t interp;                /* SARX_BALANCE_NEAREST or SARX_BALANCE_BILINEAR */
    int32_t min_count;             /* >= 1 */
    int32_t reserved;              /* 0 */
    double clip_power;             /* > 0, +inf = no clip */
    double min_coherence;          /* 0 .. 1 */
} sarx_balance_params;             /* 40 bytes */

typedef struct {
    uint32_t nb_az, nb_rg;
    uint32_t n_valid;              /* valid blocks */
    uint32_t reserved;             /* 0 */
    double w_re, w_im;             /* global weight */
    double coherence;              /* global coherence */
    double s11, s22;               /* sums of S11 and S22 over the valid blocks */
    uint64_t n;                    /* pixels kept in the valid blocks */
} sarx_balance_header;             /* 64 bytes */

typedef struct {
    double s12_re, s12_im, s11, s22;
    double w_re, w_im;             /* the block's weight, or the global one when the block is not valid */
    float coherence;
    uint32_t n;                    /* pixels kept */
    uint32_t valid;                /* 0 or 1 */
    uint32_t reserved;             /* 0 */
} sarx_balance_record;             /* 64 bytes */

/* validates the parameters for an [n_az x n_rg] image (no device needed) */
int sarx_balance_check(const sarx_balance_params* params, int n_az, int n_rg);
/* bytes of the table (header + records) and of the estimate's workspace for that image */
int sarx_balance_table_bytes(const sarx_balance_params* params, int n_az, int n_rg, size_t* out_bytes);
int sarx_balance_workspace_bytes(const sarx_balance_params* params, int n_az, int n_rg, size_t* out_bytes);
/* block sums, weights and coherence of (slc1, slc2) into d_table (8-byte aligned, as d_workspace) */
int sarx_balance_estimate_dev(sarx_ctx* ctx, const void* d_slc1, const void* d_slc2, int n_az, int n_rg,
                              const sarx_balance_params* params, void* d_table, void* d_workspace);
/* d_slc2_out = w d_slc2 with the table of an estimate call with the same params and size; d_slc2_out may be d_slc2.
 * d_dpca_mag (4-byte aligned) may be NULL; d_slc1 is read only with d_dpca_mag and may be NULL without it */
int sarx_balance_apply_dev(sarx_ctx* ctx, const void* d_slc1, const void* d_slc2, int n_az, int n_rg,
                           const sarx_balance_params* params, const void* d_table, void* d_slc2_out, float* d_dpca_mag);

#ifdef __cplusplus
}
#endif
#endif /* SARX_BALANCE_H */
