// The back-projection plan itself: what tdbp.hip, the focus-velocity search (tdbp_search.hip), the N-receiver stack (tdbp_multi.hip), its
// two-receiver case (tdbp_pair.hip) and the search on the pair per GMTI report (tdbp_pair_search.hip) share and no other unit sees: the
// plan, the geometry bounds, the scratch a unit holds (TdbpScratch; TdbpHypScratch with a hypothesis table; TdbpRx with the channels of
// a receiver stack) and the kernel arguments they have in common (tdbp_fill_args, tdbp_rx_fill_args).
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "tdbp_pixel.hpp"
#include "tdbp_multi.h"
#include "tdbp_pair.h"
#include "tdbp_pair_search.h"
#include "tdbp_search.h"

namespace sarx {

struct PulseGeo {            // one 64-byte record per pulse, read with scalar loads
    double px, py, pz;       // platform position
    double wx, wy, wz;       // platform velocity - focus velocity  (v_rel, :211)
    double dt, pad;          // t_pulse - mean(t_pulses) (:203-204); pad = |v_rel|^2
};

struct Tdbp {
    int n_p = 0, n_s = 0, nx = 0, ny = 0, taps = 0, m = 0, blk = 0, chunks = 1, per_chunk = 0;
    sarx_tdbp_params k{};
    const cf* tw_all = nullptr;
    cf *work = nullptr, *rc = nullptr;   // rc: [n_p][n_s], filled by tdbp_range_compress
    std::map<int, cf*> hhat;      // conj spectrum of the reference chirp per FFT length (device order)
    int l_ref = 0;
    bool full_rc = false;         // SARX_TDBP_FULL_RC=1: always compress every sample
    bool three_launch = false;    // SARX_TDBP_RC_FUSED=0: copy-in, two transforms, copy-out per block (the form of rounds 2-4, for A/B)
    int win_lo = 0, win_hi = 0;   // samples compressed by the last call
    // per-pulse table, double-buffered: frame i + 1's table is staged in page-locked memory and copied on the stream while frame i
    // still reads its own - no stream synchronisation per frame (the copy of rounds 2-4 was a blocking one behind a hipStreamSynchronize
    // that made the host wait for the frame's echo, noise and range compression before it could enqueue the back-projection)
    PulseGeo* geo[2] = {nullptr, nullptr};
    PulseGeo* h_geo[2] = {nullptr, nullptr};
    hipEvent_t geo_done[2] = {nullptr, nullptr};
    int geo_slot = 0;
    double *xax = nullptr, *yax = nullptr;   // pixel axes, valid after tdbp_ensure_axes
    double axes_scene = -1.0;     // scene_size the pixel axes on the device were built for
    double2 *part = nullptr, *img = nullptr;
    uint64_t bytes = 0;
    TdbpSearch* search = nullptr; // scratch of the focus-velocity search (tdbp_search.hip), made by its first call, freed by tdbp_destroy
    TdbpRx* pair = nullptr;       // scratch of the two-receiver pair, capacity 2 (tdbp_pair.hip), likewise
    TdbpPairSearch* pair_search = nullptr;   // scratch of the search on the pair (tdbp_pair_search.hip), likewise
    TdbpRx* multi = nullptr;      // scratch of the N-receiver stack, capacity MAX_RX (tdbp_multi.hip), likewise
};

#define TCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

// samples [lo, hi) of every pulse of raw, compressed into dst [n_p][n_s]: t->rc, or the pair's buffer for its second channel
hipError_t tdbp_range_compress(Tdbp* t, const float2* raw, cf* dst, int lo, int hi, hipStream_t st);
hipError_t tdbp_ensure_axes(Tdbp* t, double scene_size, hipStream_t st);
// position and dt = t_pulse - mean(t_pulses) of every pulse; then w = v_plat - vf and |w|^2 for one focus velocity
void tdbp_pulse_table(const Tdbp* t, const double* pos, const double* t_pulses, std::vector<PulseGeo>& geo);
void tdbp_set_focus(std::vector<PulseGeo>& geo, const double* vel, const double* vf);
// geo holds w = v_plat - vf for the SAME vf
void tdbp_sample_window(const Tdbp* t, const std::vector<PulseGeo>& geo, const double* vf, double t_start, double scene_size,
                        int* lo, int* hi);
bool tdbp_tile_ok(const Tdbp* t, const std::vector<PulseGeo>& geo, const double* vf, double scene_size);
// what those two bounds and the receivers' own (tdbp_pair_bounds) are made of: the transmit range of one pulse over the moved pixel rectangle of half
// side h, sample indices to a window inside [0, n_s] (NaN-safe), the farthest pixel of a tile from its reference pixel (< 0: grid too thin)
void moved_rect_range(const PulseGeo& g, const double* vf, double h, double* dmin, double* dmax);
void tdbp_clamp_window(double imin, double imax, int n_s, int* lo, int* hi);
double tdbp_tile_reach(const Tdbp* t, double scene_size);
// the receivers' own bounds over the pulses [u0, u1) for one focus velocity (tdbp_pair.hip), off_max the largest |offset|: the sample
// window any channel can touch, whether the series of tdbp_pair_pixel holds, and whether the receivers' part of the tile expansion does
void tdbp_pair_bounds(const Tdbp* t, const std::vector<PulseGeo>& geo, int u0, int u1, const double* vf, double t_start, double scene_size,
                      double off_max, double chirp_centre, int* lo, int* hi, bool* series, bool* tile);
// the receivers' table from the pulse table and the transmitter's velocity rows (none zero)
void tdbp_pair_table(PairGeo* h_geo, const std::vector<PulseGeo>& geo, const double* vel, int n_p);
// the pair scratch's buffer of channel 1's range-compressed pulses [n_p][n_s] (made with the scratch by the first call)
hipError_t tdbp_pair_rc1(Tdbp* t, cf** rc1);
// pulse chunks of one search or pair call, and the pulses in each; requested < 1: chosen here
int tdbp_pick_chunks(int tiles, int blocks_per_chunk, int n_pulses, int requested, int* per_chunk);

// What the search and the pair each hold beside the plan, made by their first call: the per-pulse table of their own record type
// (SearchGeo, PairGeo) with its page-locked staging, the partial images, and the route the last call took.
struct TdbpScratch {
    void *geo = nullptr, *h_geo = nullptr;                 // device table and its page-locked staging
    size_t bytes = 0;                                      // of either
    hipEvent_t up_done = nullptr;                          // the uploads of the last call have read the staging
    double2* part = nullptr; size_t part_cap = 0;          // partial images, grown on demand; double2 elements
    int route = -1;                                        // 1 tile form, 0 exact form, -1 no call yet
};
hipError_t tdbp_scratch_init(TdbpScratch* s, int n_p, size_t bytes);   // n_p records of bytes each
void tdbp_scratch_free(TdbpScratch* s);
hipError_t grow(double2** buf, size_t* cap, size_t need);              // *buf holds at least need elements; the old content is not kept
inline hipError_t grow_bytes(double2** buf, size_t* cap, size_t bytes) { return grow(buf, cap, (bytes + sizeof(double2) - 1) / sizeof(double2)); }
// fill writes the staging once the previous call's uploads have left it (at once as a rule) and enqueues what else it stages; the table follows
template <class F> hipError_t tdbp_scratch_upload(TdbpScratch* s, hipStream_t st, F fill) {
    TCK(hipEventSynchronize(s->up_done));
    TCK(fill(s->h_geo));
    TCK(hipMemcpyAsync(s->geo, s->h_geo, s->bytes, hipMemcpyHostToDevice, st));
    return hipEventRecord(s->up_done, st);
}
// The scratch of a search (TdbpSearch, TdbpPairSearch): the pulse table and a table of focus velocities [max_hyp][3] with its staging
struct TdbpHypScratch : TdbpScratch { double *hyps = nullptr, *h_hyps = nullptr; };
hipError_t tdbp_hyp_scratch_init(TdbpHypScratch* s, int n_p, size_t bytes, int max_hyp);
void tdbp_hyp_scratch_free(TdbpHypScratch* s);
// table writes the pulse table into its staging; the n_hyp <= max_hyp hypotheses are staged and uploaded with it
template <class F> hipError_t tdbp_hyp_upload(TdbpHypScratch* s, const double* vel_hyps, int n_hyp, hipStream_t st, F table) {
    return tdbp_scratch_upload(s, st, [&](void* staging) {
        table(staging);
        memcpy(s->h_hyps, vel_hyps, (size_t)n_hyp * 3 * sizeof(double));
        return hipMemcpyAsync(s->hyps, s->h_hyps, (size_t)n_hyp * 3 * sizeof(double), hipMemcpyHostToDevice, st);
    });
}
// the kernel arguments that the focus launch (TdbpArgs) and the search launch (SearchArgs) share
template <class A> void tdbp_fill_args(const Tdbp* t, double t_start, int per_chunk, A& a) {
    a.rc = t->rc; a.xax = t->xax; a.yax = t->yax;
    a.inv_c = 1.0 / t->k.c; a.fc = t->k.fc; a.fs = t->k.fs; a.t_start = t_start;
    a.k_shift = -t->k.fc * 2.0 / t->k.c / t->k.k_rate;
    a.inv_ns = 1.0 / (double)t->n_s; a.half_w = (float)t->n_s / 2.0f;
    a.n_p = t->n_p; a.n_s = t->n_s; a.nx = t->nx; a.ny = t->ny; a.per_chunk = per_chunk;
}
// What a receiver stack holds beside the plan (tdbp_multi.hip): the PairGeo table, the range-compressed pulses of channels 1 and up
// (channel 0's are the plan's) with the raw staging of the host entry point, each made when first used, and both output forms.  The
// plan keeps two: t->pair of capacity 2, which the pair's calls run on and whose channel 1 serves the pair's search, and t->multi of
// capacity MAX_RX for the stack's calls - so each answers for its own calls only and a pair-only plan holds two channels' memory.
struct TdbpRx : TdbpScratch {
    int cap = 0;                                           // channels, fixed when made
    cf* rc[MAX_RX - 1] = {};                               // [n_p][n_s] range-compressed pulses of channels 1 .. cap - 1
    float2* raw[MAX_RX - 1] = {};                          // staging of the host entry point, likewise
    double2* img128 = nullptr;                             // [cap][ny*nx]
    float2* img64 = nullptr;
};
// inst: t->pair or t->multi, made here with cap channels when NULL; then the compressed buffers of n_rx <= cap channels
hipError_t tdbp_rx_scratch(Tdbp* t, TdbpRx*& inst, int cap, int n_rx, TdbpRx** out);
void tdbp_rx_free(TdbpRx* s);
// device staging of a host entry point: the raw pulses of channels 1 .. n_rx - 1 [n_p][n_s] and both output forms [cap][ny][nx]
hipError_t tdbp_rx_staging(Tdbp* t, TdbpRx*& inst, int cap, int n_rx, float2** d_raw, double2** d_img128, float2** d_img64);
// bytes s holds on the device and a sum over its buffers' addresses (0, 0 for NULL)
void tdbp_rx_held(const Tdbp* t, const TdbpRx* s, uint64_t* bytes, uint64_t* id);
// the back-projection of prm->n_rx <= cap channels on inst; the arguments of tdbp_multi (tdbp_multi.h)
hipError_t tdbp_rx(Tdbp* t, TdbpRx*& inst, int cap, const float2* const* raw, const double* pos, const double* vel, const double* t_pulses,
                   double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* prm, int chunks,
                   double2* d_img128, float2* d_img64, hipStream_t st);
// What the parameters and the plan say of the arguments the receivers' loops read (RxArgs, tdbp_pixel.hpp), the union [u0, u1) of the
// channels' pulse ranges among them; where the pulses and the table lie (rc, geo) the caller sets from the scratch it holds.
inline void tdbp_rx_fill_args(const Tdbp* t, double t_start, const sarx_tdbp_multi_params* prm, RxArgs& a) {
    a.u0 = a.u1 = prm->first_pulse[0];
    for (int c = 0; c < prm->n_rx; ++c) {
        a.off[c] = prm->rx_offset_m[c]; a.first[c] = prm->first_pulse[c];
        if (a.first[c] < a.u0) a.u0 = a.first[c];
        if (a.first[c] > a.u1) a.u1 = a.first[c];
    }
    a.u1 += prm->n_used;
    a.n_used = prm->n_used;
    a.fc = t->k.fc; a.half_w = (float)t->n_s / 2.0f; a.n_s = t->n_s;
    a.inv_c = 1.0 / t->k.c; a.fs = t->k.fs; a.t_start = t_start; a.chirp_centre = prm->chirp_centre_s; a.inv_ns = 1.0 / (double)t->n_s;
}
// the largest |offset| of the channels: all that tdbp_pair_bounds reads of them
inline double tdbp_rx_off_max(const RxArgs& a, int n_rx) {
    double om = 0.0;
    for (int c = 0; c < n_rx; ++c) om = fmax(om, fabs(a.off[c]));
    return om;
}
}  // namespace sarx
