/* libsarx two-receiver back-projection: both receive channels of the two-receiver echo model (sar_ati_dcpa_sim_csa.py:113-178)
 * imaged onto ONE ground grid in one launch, so the pair is co-registered pixel for pixel with no resampling and goes straight
 * into the ATI / DPCA products and the GMTI chain.  The ATI phase of a pixel is
 * angle(I0 conj(I1)) = -4 pi v_los lag / lambda with lag = (off1 - off0) / (2 |v_tx|): the radial speed the focus-velocity
 * search of sarx_tdbp_search.h cannot see.
 *
 * Plain C99.  Extends include/sarx.h: the context, the error codes, sarx_tdbp_plan and the argument conventions of
 * sarx_tdbp_focus_dev / _host come from there.
 *
 *    per channel c, pixel (x_i, y_j) (axes as sarx_tdbp_focus_*) and used pulse p, in rising p:
 *        dt    = t_pulses[p] - mean(t_pulses)                 the mean over ALL n_pulses, one definition for both channels
 *        g     = (x_i, y_j, 0) + vel_focus dt
 *        p_rx  = pos_tx[p] + rx_offset_m[c] vel_tx[p] / |vel_tx[p]|
 *        tau   = (|g - pos_tx[p]| + |g - p_rx|) / C           no stop-and-go receiver, no Doppler time shift
 *        idx_f = (tau - t_start + chirp_centre_s) FS
 *        xn    = float32(2 idx_f / num_samples - 1), read as F.grid_sample reads it (two taps, zeros outside)
 *        I_c  += sample * exp(j 2 pi FC tau)                  summed in fp64
 *    range compression : the plan's, once per channel, over a sample window that is a geometric bound of what the pixels can
 *                        touch (every sample with SARX_TDBP_FULL_RC=1, as for sarx_tdbp_focus_*).
 *    geometry          : exact per pixel and pulse (one reciprocal square root for both channels), or expanded about the reference
 *                        pixel of each 16 x 16 tile as sarx_tdbp_focus_* does it, when the truncation error of the expansion is
 *                        bounded below 1e-9 m over all pulses for both channels; sarx_tdbp_pair_route tells which ran.
 *                        SARX_TDBP_TILE=0 forces the exact form here as it does there.
 *    determinism       : pulse chunks summed in chunk order, no atomics: the same bits from run to run.  The number of chunks is
 *                        chosen from the grid size, or is what sarx_tdbp_search_set_chunks (sarx_tdbp_search.h) set on the plan.
 *    scratch           : belongs to the plan; made by the first call, a repeated call allocates nothing on the device.  As with
 *                        sarx_tdbp_focus_dev, a plan serves one lane at a time.
 *
 * More than two receivers: sarx_tdbp_multi.h.  Left out: a velocity search on the pair, relocating movers on the ground grid, fusing the ATI / DPCA
 * planes into the reduce launch. */
#ifndef SARX_TDBP_PAIR_H
#define SARX_TDBP_PAIR_H

#include "sarx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    double rx_offset_m[2];         /* receiver of channel c at pos_tx + rx_offset_m[c] * unit(vel_tx); finite */
    double chirp_centre_s;         /* where the compressed peak sits relative to the delay: 0 for a chirp centred on tau
                                      (run_physics_spotlight), T_p / 2 for one that starts at tau (run_bistatic_physics_gpu) */
    int32_t first_pulse[2];        /* channel c uses pulses first_pulse[c] .. first_pulse[c] + n_used - 1 */
    int32_t n_used;                /* DPCA pulse shift: first_pulse {1, 0}, n_used n_pulses - 1; none: {0, 0}, n_pulses */
    int32_t reserved;              /* 0 */
} sarx_tdbp_pair_params;           /* 40 bytes */

/* params alone against a pulse count: SARX_OK, or SARX_ERR_INVALID and a message in sarx_last_error(NULL).  Needs no device. */
int sarx_tdbp_pair_check(int n_pulses, const sarx_tdbp_pair_params* params);
/* d_raw0, d_raw1: device complex64 [n_pulses][num_samples]; pos_tx, vel_tx [n_pulses][3], t_pulses [n_pulses], vel_focus [3]:
 * host fp64, no vel_tx row zero.  d_images128: device complex128 [2][ny][nx] or NULL (16-byte aligned); d_images64: device
 * complex64 [2][ny][nx] or NULL (8-byte aligned), the fp64 sums rounded once; not both NULL.  Returns after the small upload is
 * enqueued; everything runs on the ctx's current lane. */
int sarx_tdbp_pair_dev(sarx_tdbp_plan* plan, const void* d_raw0, const void* d_raw1, const double* pos_tx, const double* vel_tx,
                       const double* t_pulses, double t_start, const double* vel_focus, double scene_size,
                       const sarx_tdbp_pair_params* params, void* d_images128, void* d_images64);
/* blocking; raw0, raw1, images128 (or NULL) and images64 (or NULL) are host memory */
int sarx_tdbp_pair_host(sarx_tdbp_plan* plan, const void* raw0, const void* raw1, const double* pos_tx, const double* vel_tx,
                        const double* t_pulses, double t_start, const double* vel_focus, double scene_size,
                        const sarx_tdbp_pair_params* params, void* images128, void* images64);
/* *tile = 1 when the plan's last pair call took the tile-expanded kernel, 0 for the exact one; SARX_ERR_INVALID before any pair call */
int sarx_tdbp_pair_route(const sarx_tdbp_plan* plan, int* tile);

#ifdef __cplusplus
}
#endif
#endif /* SARX_TDBP_PAIR_H */
