/* libsarx N-receiver back-projection and the multi-baseline ATI resolver.
 *
 * 1. sarx_tdbp_multi_*: n_rx = 2, 3 or 4 receive channels of the bistatic echo model (run_bistatic_physics_gpu,
 *    sar_ati_dcpa_sim_csa.py:107-178, one call per receiver offset) imaged onto ONE ground grid in one enqueue: a co-registered
 *    stack.  The semantics are those of sarx_tdbp_pair.h, per channel c, pixel (x_i, y_j) and used pulse p, in rising p:
 *        dt    = t_pulses[p] - mean(t_pulses)                 the mean over ALL n_pulses, one definition for every channel
 *        g     = (x_i, y_j, 0) + vel_focus dt
 *        p_rx  = pos_tx[p] + rx_offset_m[c] vel_tx[p] / |vel_tx[p]|
 *        tau   = (|g - pos_tx[p]| + |g - p_rx|) / C           no stop-and-go receiver, no Doppler time shift
 *        idx_f = (tau - t_start + chirp_centre_s) FS
 *        xn    = float32(2 idx_f / num_samples - 1), read as F.grid_sample reads it (two taps, zeros outside)
 *        I_c  += sample * exp(j 2 pi FC tau)                  summed in fp64
 *    pulse ranges      : channel c uses pulses first_pulse[c] .. first_pulse[c] + n_used - 1.
 *    range compression : the plan's, once per channel, over ONE sample window that bounds what any channel can touch (every sample
 *                        with SARX_TDBP_FULL_RC=1).
 *    geometry          : exact per pixel and pulse (the transmit leg once for all channels), or expanded about the reference pixel
 *                        of each 16 x 16 tile when the pair's truncation bounds hold below 1e-9 m for every channel (taken with the
 *                        largest |rx_offset_m|); sarx_tdbp_multi_route tells which ran.  SARX_TDBP_TILE=0 forces the exact form.
 *    determinism       : pulse chunks summed in chunk order, no atomics: the same bits from run to run.  The number of chunks is
 *                        chosen from the grid size, or is what sarx_tdbp_search_set_chunks (sarx_tdbp_search.h) set on the plan.
 *                        With n_rx = 2 the two images are the bits of sarx_tdbp_pair_* for the same arguments.
 *    scratch           : belongs to the plan; made by the first call with a given n_rx, a repeated call allocates nothing on the
 *                        device.  A plan serves one lane at a time.
 *
 * 2. sarx_tdbp_multi_resolve_*: one radial speed per GMTI report from the n_rx - 1 baselines of the stack.  Baseline b is the
 *    channel pair (0, b + 1) with lag_s[b] = (off_{b+1} - off_0) / (2 |v_tx|); its ATI phase measures the speed modulo
 *    lambda / (2 |lag_b|).  A short baseline is unambiguous but insensitive, a long one sensitive but wrapped: the wrap count of
 *    the longest baseline is the one under which the other baselines agree best (the search of the reference's CRT Solver demo,
 *    CRT Solver.html:40-51, with the long baseline as the ruler).  Per report at (i, j) of the slot (count read on the device: no
 *    host round trip, no atomics), everything in fp64:
 *        W_b    = sum I_0 conj(I_{b+1}) over the box |di| <= half, |dj| <= half clipped to the image, rows rising, then columns
 *                 rising; every term the exact fp64 product of two fp32 samples
 *        phi_b  = atan2(Im W_b, Re W_b)
 *        B      = the baseline of largest |lag_b| (ties: the smaller b);  S = that of smallest |lag_b| (ties: the smaller b)
 *        v_k    = -lambda (phi_B + 2 pi k) / (4 pi lag_B);  the candidates are the integers k with |v_k| <= v_max_mps
 *        J(k)   = sum over b != B of wrap(phi_b + 4 pi lag_b v_k / lambda)^2,  wrap(x) = x - 2 pi ceil((x - pi) / (2 pi)) onto (-pi, pi]
 *        k      = the candidate of least J; ties go to the smaller |k|, then to k >= 0
 *    record: v_los = v_k; v_coarse = -lambda phi_S / (4 pi lag_S); cost = J(k); cost_next = the least J among the other candidates
 *    (+inf with a single candidate); phase[b] = phi_b (0 for b >= n_rx - 1); status SARX_TDBP_MULTI_OK.
 *        no candidate inside v_max_mps : status _NO_CANDIDATE; phases and v_coarse as above, v_los = 0, k = 0, cost = cost_next = +inf
 *        a W_b exactly zero (an empty box, too: a report whose box misses the image) : status _ZERO; phases as above, every other field 0
 *        the slot's overflow flag set or count > max_detections : record 0 alone is written, every field 0 but status _OVERFLOW
 *                 (as sarx_atigate.h and sarx_cluster.h treat it: an error, never a truncated answer)
 *    With n_rx = 2 there is one baseline: J = 0, k = 0 when |v_0| <= v_max_mps, and v_los is the plain ATI speed.
 *    Nothing past 64 count bytes of the records is touched.
 *
 * Plain C99.  Extends include/sarx.h and include/sarx_gmti.h (the context, the error codes, sarx_tdbp_plan, the slot layout).
 *
 * The records feed sarx_relocate.h as they lie on the device (v_los at offset 0, status at offset 60, stride 64): each report is
 * put back at its ground position, and the relocated list is a slot the tracker takes.
 *
 * Left out: the focus-velocity search on N channels, coherence-weighted costs, a maximum-likelihood combination of the baselines
 * after unwrapping. */
#ifndef SARX_TDBP_MULTI_H
#define SARX_TDBP_MULTI_H

#include "sarx.h"
#include "sarx_gmti.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_TDBP_MULTI_MAX_RX 4
#define SARX_TDBP_MULTI_MAX_HALF 4
#define SARX_TDBP_MULTI_MAX_CANDIDATES 129
#define SARX_TDBP_MULTI_MAX_DETECTIONS 16384
#define SARX_TDBP_MULTI_MAX_DIM (1 << 20)  /* ny and nx of the resolver's stack: 8 n_rx ny nx stays below 2^45 bytes */

#define SARX_TDBP_MULTI_OK 0u
#define SARX_TDBP_MULTI_NO_CANDIDATE 1u
#define SARX_TDBP_MULTI_ZERO 2u
#define SARX_TDBP_MULTI_OVERFLOW 3u

typedef struct {
    double rx_offset_m[4];         /* receiver of channel c at pos_tx + rx_offset_m[c] * unit(vel_tx); finite; 0 for c >= n_rx */
    double chirp_centre_s;         /* as in sarx_tdbp_pair_params */
    int32_t first_pulse[4];        /* channel c uses pulses first_pulse[c] .. first_pulse[c] + n_used - 1; 0 for c >= n_rx */
    int32_t n_used;
    int32_t n_rx;                  /* 2 .. SARX_TDBP_MULTI_MAX_RX */
} sarx_tdbp_multi_params;          /* 64 bytes */

typedef struct {
    double lag_s[3];               /* baseline b = channels (0, b + 1): finite and non-zero for b < n_rx - 1, 0 beyond */
    double wavelength_m;           /* finite, > 0 */
    double v_max_mps;              /* finite, > 0: the largest |v_los| a candidate may have */
    int32_t n_rx;                  /* 2 .. SARX_TDBP_MULTI_MAX_RX */
    int32_t half;                  /* window half-width 0 .. SARX_TDBP_MULTI_MAX_HALF; 1 gives the 3 x 3 of the report */
    int32_t max_detections;        /* capacity of the slot, 1 .. SARX_TDBP_MULTI_MAX_DETECTIONS */
    int32_t reserved;              /* 0 */
} sarx_tdbp_multi_resolve_params;  /* 56 bytes */

typedef struct {
    double v_los, v_coarse, cost, cost_next;
    double phase[3];
    int32_t k;
    uint32_t status;               /* SARX_TDBP_MULTI_OK / _NO_CANDIDATE / _ZERO / _OVERFLOW */
} sarx_tdbp_multi_record;          /* 64 bytes */

/* params alone against a pulse count: SARX_OK, or SARX_ERR_INVALID and a message in sarx_last_error(NULL).  Needs no device. */
int sarx_tdbp_multi_check(int n_pulses, const sarx_tdbp_multi_params* params);
/* d_raw: HOST array of n_rx device pointers, each complex64 [n_pulses][num_samples]; pos_tx, vel_tx [n_pulses][3], t_pulses
 * [n_pulses], vel_focus [3]: host fp64, no vel_tx row zero.  d_images128: device complex128 [n_rx][ny][nx] or NULL (16-byte
 * aligned); d_images64: device complex64 [n_rx][ny][nx] or NULL (8-byte aligned), the fp64 sums rounded once; not both NULL.
 * Returns after the small upload is enqueued; everything runs on the ctx's current lane. */
int sarx_tdbp_multi_dev(sarx_tdbp_plan* plan, const void* const* d_raw, const double* pos_tx, const double* vel_tx, const double* t_pulses,
                        double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* params,
                        void* d_images128, void* d_images64);
/* blocking; raw: array of n_rx host pointers; images128 (or NULL) and images64 (or NULL) are host memory */
int sarx_tdbp_multi_host(sarx_tdbp_plan* plan, const void* const* raw, const double* pos_tx, const double* vel_tx, const double* t_pulses,
                         double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* params,
                         void* images128, void* images64);
/* *tile = 1 when the plan's last multi call took the tile-expanded kernel, 0 for the exact one; SARX_ERR_INVALID before any */
int sarx_tdbp_multi_route(const sarx_tdbp_plan* plan, int* tile);
/* Diagnostic only (the tests' evidence that a repeated call allocates nothing; no caller needs it to run the stack): what the
 * plan's multi scratch holds on the device, *bytes in all (0 before any multi call), and *id, a sum over its buffers' addresses.
 * Both equal before and after a call: no buffer was added and none grew.  A sum cannot tell a buffer freed and made again at its
 * old address, which the scratch never does (its buffers are made once or grow, they are not freed before the plan is). */
int sarx_tdbp_multi_scratch(const sarx_tdbp_plan* plan, uint64_t* bytes, uint64_t* id);

/* validates the resolver's parameters (no device needed); refuses those that allow more than SARX_TDBP_MULTI_MAX_CANDIDATES */
int sarx_tdbp_multi_resolve_check(const sarx_tdbp_multi_resolve_params* params);
/* d_images64: device complex64 [n_rx][ny][nx] (8-byte aligned; ny, nx 1 .. SARX_TDBP_MULTI_MAX_DIM); d_slot: a GMTI slot of
 * max_detections reports (8-byte aligned), i = row 0 .. ny - 1, j = column 0 .. nx - 1; d_records: max_detections
 * sarx_tdbp_multi_record (8-byte aligned), which may overlap neither input.  One launch on the ctx's current lane, only enqueued. */
int sarx_tdbp_multi_resolve_dev(sarx_ctx* ctx, const sarx_tdbp_multi_resolve_params* params, const void* d_images64, int ny, int nx,
                                const void* d_slot, void* d_records);

#ifdef __cplusplus
}
#endif
#endif /* SARX_TDBP_MULTI_H */
