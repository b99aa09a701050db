// Focus-velocity search on the two-receiver back-projection, per GMTI report: for every report of a GMTI slot on the
// device and every one of n_hyp focus velocities, both receive channels imaged on a chip of the pair's grid around the report, the
// chip's DPCA difference folded into one record, the best hypothesis named per report and the ATI interferogram taken at its peak.
//
//   1 range compression, once per channel: tdbp_range_compress over ONE sample window, the union over the hypotheses of the pair's
//     bound (tdbp_pair_bounds) over the whole grid - the chips are not known on the host.  Channel 0 lands in the plan's rc buffer,
//     channel 1 in the pair scratch's.
//   2 back-projection: grid (tiles of the chip) x (report * n_hyp + hypothesis) x (pulse chunk), one thread per chip pixel carrying
//     BOTH channels through the pulse loops tdbp_multi.hip's kernels run, at N = 2 (tdbp_multi_pulses, tdbp_multi_tile_pulses of tdbp_pixel.hpp).
//     A workgroup reads the slot's header and its report: past the count, on an overflowed slot or with the report outside the grid
//     it leaves at once (before any barrier; the test is workgroup-uniform).  Partial chips [max_det][n_hyp][chunks][2][chip_y * chip_x].
//     The exact form (tdbp_pair_search_kernel) and the one expanded about the reference pixel of each 16 x 16 tile OF THE CHIP
//     (tdbp_pair_search_tile_kernel): tdbp_pix and tdbp_tile_offsets of tdbp_pixel.hpp on the chip's extent and the axis tables shifted to
//     the chip's corner, so a pixel is never farther from its reference pixel than the grid's tiles allow and tdbp_tile_ok and the
//     pair's remainder bound, evaluated over the whole grid for every hypothesis, cover every chip.
//   3 metric launch, one 256-thread workgroup per (report, hypothesis): the chunks of every chip pixel summed in chunk order for both
//     channels, the chip written when asked for, and P = |D|^2 (D = I0 - I1 or I0; products and sum rounded one by one) folded into s2,
//     s4, the peak and its place: thread t takes pixels t, t + 256, ... in rising order, then a binary tree over the 256 threads in LDS.
//   4 best launch, one wave per report: k_best = argmax s4 over the hypotheses (a lane each, a butterfly over the wave), its neighbours'
//     s4, and the 3 x 3 interferogram around the peak of k_best from the partial chips, summed again in chunk order (a lane per pixel
//     and channel) and added in a fixed order.
// No atomics and no host round trip: the same bits on every run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "gmti_dev.hpp"
#include "tdbp_plan.h"

namespace sarx {

static_assert(sizeof(sarx_tdbp_pair_search_params) == 16, "sarx_tdbp_pair_search_params is 16 bytes");
static_assert(sizeof(sarx_tdbp_pair_search_best) == 80, "sarx_tdbp_pair_search_best is 80 bytes");
static_assert(sizeof(sarx_tdbp_search_record) == 32, "sarx_tdbp_search_record is 32 bytes");

struct PairSearchArgs : RxArgs {     // channels 0 and 1
    const double* hyps;              // [n_hyp][3]
    const double *xax, *yax;
    const sarx_gmti_report* rep;
    const sarx_gmti_header* hdr;
    double2* part;                   // [max_det][n_hyp][chunks][2][chip_y * chip_x]
    sarx_tdbp_search_record* rec;    // [max_det][n_hyp]
    sarx_tdbp_pair_search_best* best;   // [max_det]
    double2* chips;                  // [max_det][n_hyp][2][chip_y * chip_x] or NULL
    int nx, ny, chip_x, chip_y, n_hyp, max_det, source, per_chunk, chunks;
};

// What a workgroup does for report r: nothing (past the count, or the slot is unusable), k_best = -1 (the report lies outside the
// grid), or the chip at (x0, y0).  The same for every thread of the workgroup.
enum { CHIP_SKIP = 0, CHIP_OUTSIDE = 1, CHIP_RUN = 2 };
__device__ __forceinline__ int chip_of(const PairSearchArgs& a, int r, int& x0, int& y0) {
    const SlotView s = slot_view(a.hdr, a.max_det);      // count and unusable only: the reports come as a.rep
    if (s.unusable || (uint32_t)r >= s.count) return CHIP_SKIP;
    const int i = a.rep[r].i, j = a.rep[r].j;
    if (i < 0 || i >= a.ny || j < 0 || j >= a.nx) return CHIP_OUTSIDE;
    x0 = min(max(j - a.chip_x / 2, 0), a.nx - a.chip_x);
    y0 = min(max(i - a.chip_y / 2, 0), a.ny - a.chip_y);
    return CHIP_RUN;
}

// the partial chip of channel ch of this workgroup's (report, hypothesis) = blockIdx.y and chunk = blockIdx.z
__device__ __forceinline__ void store_partial(const PairSearchArgs& a, const TdbpPix& px, const double (&re)[2], const double (&im)[2]) {
    if (!px.live) return;
    const size_t n_chip = (size_t)a.chip_x * a.chip_y;
    const size_t at = ((size_t)blockIdx.y * a.chunks + blockIdx.z) * 2 * n_chip + (size_t)px.iy * a.chip_x + px.ix;
    a.part[at] = make_double2(re[0], im[0]);
    a.part[at + n_chip] = make_double2(re[1], im[1]);
}

template <bool SERIES> __global__ __launch_bounds__(256) void tdbp_pair_search_kernel(PairSearchArgs a) {
    const int r = blockIdx.y / a.n_hyp, h = blockIdx.y - r * a.n_hyp;
    int x0 = 0, y0 = 0;
    if (chip_of(a, r, x0, y0) != CHIP_RUN) return;
    const TdbpPix px = tdbp_pix(a.chip_x, a.chip_y);      // chip coordinates
    const double gx0 = a.xax[x0 + (px.live ? px.ix : 0)], gy0 = a.yax[y0 + (px.live ? px.iy : 0)];
    const double vfx = a.hyps[3 * h], vfy = a.hyps[3 * h + 1], vfz = a.hyps[3 * h + 2];
    const int p0 = a.u0 + blockIdx.z * a.per_chunk, p1 = min(a.u1, p0 + a.per_chunk);
    double re[2] = {}, im[2] = {};
    tdbp_multi_pulses<2, SERIES>(a, vfx, vfy, vfz, gx0, gy0, p0, p1, re, im);
    store_partial(a, px, re, im);
}

// the tile form on the chip's own tiles: the axis tables shifted to the chip's corner, the chip's extent as the grid
__global__ __launch_bounds__(256) void tdbp_pair_search_tile_kernel(PairSearchArgs a) {
    __shared__ MultiTilePulse<2> s_tp[TP_BATCH];
    const int r = blockIdx.y / a.n_hyp, h = blockIdx.y - r * a.n_hyp;
    int x0 = 0, y0 = 0;
    if (chip_of(a, r, x0, y0) != CHIP_RUN) return;        // the whole workgroup, before the first barrier
    const TdbpPix px = tdbp_pix(a.chip_x, a.chip_y);
    const TdbpTileOffsets o = tdbp_tile_offsets(a.xax + x0, a.yax + y0, px, a.chip_x, a.chip_y);
    const double vfx = a.hyps[3 * h], vfy = a.hyps[3 * h + 1], vfz = a.hyps[3 * h + 2];
    const int p0 = a.u0 + blockIdx.z * a.per_chunk, p1 = min(a.u1, p0 + a.per_chunk);
    double re[2] = {}, im[2] = {};
    tdbp_multi_tile_pulses<2>(a, s_tp, vfx, vfy, vfz, o, p0, p1, re, im);
    store_partial(a, px, re, im);
}

static constexpr int PM = 256;
static constexpr unsigned NO_CHIP_PIXEL = ~0u;

// One workgroup per (report, hypothesis) = blockIdx.x.  The fold is tdbp_search_metric_kernel's on 256 threads and a 32-bit index, and
// stays written out in both: as one shared function it moved this kernel's code and time (profiles/r21_tdbp_loops_resource_usage.txt).
__global__ __launch_bounds__(PM) void tdbp_pair_search_metric_kernel(PairSearchArgs a) {
    __shared__ double s_s2[PM], s_s4[PM], s_pk[PM];
    __shared__ unsigned s_at[PM];
    const int r = blockIdx.x / a.n_hyp;
    int x0 = 0, y0 = 0;
    if (chip_of(a, r, x0, y0) != CHIP_RUN) return;
    const int t = threadIdx.x;
    const unsigned n_chip = (unsigned)(a.chip_x * a.chip_y);
    const double2* src = a.part + (size_t)blockIdx.x * a.chunks * 2 * n_chip;
    double s2 = 0.0, s4 = 0.0, pk = -1.0;
    unsigned at = NO_CHIP_PIXEL;
    for (unsigned i = t; i < n_chip; i += PM) {
        const double2 z0 = tdbp_sum_chunks(src, a.chunks, 2 * (size_t)n_chip, i);
        const double2 z1 = tdbp_sum_chunks(src + n_chip, a.chunks, 2 * (size_t)n_chip, i);
        if (a.chips) {
            a.chips[(size_t)blockIdx.x * 2 * n_chip + i] = z0;
            a.chips[((size_t)blockIdx.x * 2 + 1) * n_chip + i] = z1;
        }
        const double re = a.source == SARX_TDBP_PAIR_SEARCH_DPCA ? z0.x - z1.x : z0.x;
        const double im = a.source == SARX_TDBP_PAIR_SEARCH_DPCA ? z0.y - z1.y : z0.y;
        const double p = __dadd_rn(__dmul_rn(re, re), __dmul_rn(im, im));
        s2 = __dadd_rn(s2, p);
        s4 = __dadd_rn(s4, __dmul_rn(p, p));
        if (p > pk) { pk = p; at = i; }                    // rising i: the first of equal maxima stays
    }
    s_s2[t] = s2; s_s4[t] = s4; s_pk[t] = pk; s_at[t] = at;
    __syncthreads();
    for (int s = PM / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_s2[t] = __dadd_rn(s_s2[t], s_s2[t + s]);
            s_s4[t] = __dadd_rn(s_s4[t], s_s4[t + s]);
            const double o = s_pk[t + s];
            const unsigned oa = s_at[t + s];
            if (o > s_pk[t] || (o == s_pk[t] && oa < s_at[t])) { s_pk[t] = o; s_at[t] = oa; }
        }
        __syncthreads();
    }
    if (t == 0) {
        sarx_tdbp_search_record rc;
        rc.s2 = s_s2[0]; rc.s4 = s_s4[0];
        if (s_at[0] == NO_CHIP_PIXEL) {                    // no pixel compared greater than -1: every power is NaN
            rc.peak = s_s2[0]; rc.peak_ix = -1; rc.peak_iy = -1;
        } else {                                           // the chip's rows and columns rise with the grid's: the same tie order
            rc.peak = s_pk[0];
            rc.peak_ix = x0 + (int32_t)(s_at[0] % (unsigned)a.chip_x);
            rc.peak_iy = y0 + (int32_t)(s_at[0] / (unsigned)a.chip_x);
        }
        a.rec[blockIdx.x] = rc;
    }
}

// One wave per report = blockIdx.x.  Lane h holds the s4 of hypothesis h (the n_hyp <= 64 records of the metric launch; the lanes past
// them repeat the last one), a butterfly over the wave leaves every lane with the best: the greater s4, a NaN gives way to any number,
// of equal ones (or of NaNs alone) the smaller h - a total order, so the exchange partners agree.  Lanes 0 .. 17 then sum the chunks
// of one channel of one pixel of the 3 x 3 neighbourhood each, and every lane adds the nine products in the same fixed order.
__global__ __launch_bounds__(64) void tdbp_pair_search_best_kernel(PairSearchArgs a) {
    const int r = blockIdx.x, lane = threadIdx.x;
    int x0 = 0, y0 = 0;
    const int what = chip_of(a, r, x0, y0);
    if (what == CHIP_SKIP) return;
    if (what == CHIP_OUTSIDE) { if (lane == 0) a.best[r].k_best = -1; return; }
    const int mine = min(lane, a.n_hyp - 1);
    const sarx_tdbp_search_record own = a.rec[(size_t)r * a.n_hyp + mine];
    double sb = own.s4;
    int kb = mine;
    for (int d = 32; d > 0; d >>= 1) {
        const double so = __shfl_xor(sb, d);
        const int ko = __shfl_xor(kb, d);
        const bool tie = so == sb || (so != so && sb != sb);
        if (so > sb || (sb != sb && so == so) || (tie && ko < kb)) { sb = so; kb = ko; }
    }
    sarx_tdbp_pair_search_best b;
    b.k_best = kb; b.x0 = x0; b.y0 = y0;
    b.peak_ix = __shfl(own.peak_ix, kb); b.peak_iy = __shfl(own.peak_iy, kb); b.reserved = 0;
    const double prev = __shfl(own.s4, max(kb - 1, 0)), next = __shfl(own.s4, min(kb + 1, a.n_hyp - 1)), peak = __shfl(own.peak, kb);
    b.s4_prev = kb > 0 ? prev : -1.0;
    b.s4_best = sb;
    b.s4_next = kb + 1 < a.n_hyp ? next : -1.0;
    if (b.peak_ix < 0) {                                   // every power is NaN: so is what hangs on the peak
        b.interf_re = b.interf_im = b.p0 = b.p1 = peak;
    } else {
        const size_t n_chip = (size_t)a.chip_x * a.chip_y;
        const double2* src = a.part + ((size_t)r * a.n_hyp + kb) * a.chunks * 2 * n_chip;
        const int cx = b.peak_ix - x0, cy = b.peak_iy - y0;
        // lane 2 q + c: channel c of neighbour q (rows then columns); outside the chip: nothing is read
        const int q = lane >> 1, qy = cy - 1 + q / 3, qx = cx - 1 + q % 3;
        double2 z = make_double2(0.0, 0.0);
        if (lane < 18 && qy >= 0 && qy < a.chip_y && qx >= 0 && qx < a.chip_x)
            z = tdbp_sum_chunks(src + (lane & 1) * n_chip, a.chunks, 2 * n_chip, (size_t)qy * a.chip_x + qx);
        double re = 0.0, im = 0.0;
        for (int n = 0; n < 9; ++n) {
            const double2 z0 = make_double2(__shfl(z.x, 2 * n), __shfl(z.y, 2 * n)), z1 = make_double2(__shfl(z.x, 2 * n + 1), __shfl(z.y, 2 * n + 1));
            const int ny = cy - 1 + n / 3, nx = cx - 1 + n % 3;
            if (ny < 0 || ny >= a.chip_y || nx < 0 || nx >= a.chip_x) continue;     // the same for every lane
            re += z0.x * z1.x + z0.y * z1.y;
            im += z0.y * z1.x - z0.x * z1.y;
            if (n == 4) {
                b.p0 = z0.x * z0.x + z0.y * z0.y;
                b.p1 = z1.x * z1.x + z1.y * z1.y;
            }
        }
        b.interf_re = re; b.interf_im = im;
    }
    if (lane == 0) a.best[r] = b;
}

struct TdbpPairSearch : TdbpHypScratch {                   // the table holds PairGeo
    // staging of the host entry point, in double2 elements as grow counts them
    double2 *raw1 = nullptr, *slot = nullptr, *rec = nullptr, *best = nullptr, *chips = nullptr;
    size_t raw1_cap = 0, slot_cap = 0, rec_cap = 0, best_cap = 0, chips_cap = 0;
};

void tdbp_pair_search_free(TdbpPairSearch* s) {
    if (!s) return;
    tdbp_hyp_scratch_free(s);
    hipFree(s->raw1); hipFree(s->slot); hipFree(s->rec); hipFree(s->best); hipFree(s->chips);
    delete s;
}

static hipError_t pair_search_scratch(Tdbp* t, TdbpPairSearch** out) {
    if (!t->pair_search) {
        TdbpPairSearch* s = new TdbpPairSearch();
        const hipError_t e = tdbp_hyp_scratch_init(s, t->n_p, sizeof(PairGeo), SARX_TDBP_PAIR_SEARCH_MAX_HYP);
        if (e != hipSuccess) { tdbp_pair_search_free(s); return e; }
        t->pair_search = s;
    }
    *out = t->pair_search;
    return hipSuccess;
}

hipError_t tdbp_pair_search(Tdbp* t, const float2* raw0, const float2* raw1, const double* pos, const double* vel, const double* t_pulses,
                            double t_start, double scene_size, const sarx_tdbp_pair_params* prm, const double* vel_hyps,
                            const sarx_gmti_report* d_reports, const sarx_gmti_header* d_header, int max_det,
                            const sarx_tdbp_pair_search_params* sp, int chunks, sarx_tdbp_search_record* d_records,
                            sarx_tdbp_pair_search_best* d_best, double2* d_chips, std::string* why, hipStream_t st) {
    const int n_p = t->n_p, n_hyp = sp->n_hyp;
    const sarx_tdbp_multi_params m = tdbp_pair_as_multi(*prm);
    PairSearchArgs a{};
    tdbp_rx_fill_args(t, t_start, &m, a);
    const int u0 = a.u0, u1 = a.u1;
    const double off_max = tdbp_rx_off_max(a, 2);
    // pulse chunks over the union's pulses, one chunk launching tiles x max_det x n_hyp workgroups; the partial chips must fit the cap
    const int tiles = ((sp->chip_x + 15) / 16) * ((sp->chip_y + 15) / 16);
    const size_t n_chip = (size_t)sp->chip_x * sp->chip_y;
    const size_t per_chunk_bytes = (size_t)max_det * n_hyp * 2 * n_chip * sizeof(double2);
    int per_chunk = 0;
    int n_chunks = tdbp_pick_chunks(tiles, max_det * n_hyp, u1 - u0, chunks, &per_chunk);
    while (chunks < 1 && n_chunks > 1 && per_chunk_bytes * n_chunks > SARX_TDBP_PAIR_SEARCH_MAX_PARTIAL_BYTES)
        n_chunks = tdbp_pick_chunks(tiles, max_det * n_hyp, u1 - u0, n_chunks - 1, &per_chunk);
    if (per_chunk_bytes * n_chunks > SARX_TDBP_PAIR_SEARCH_MAX_PARTIAL_BYTES) {
        char msg[320];
        snprintf(msg, sizeof msg,
                 "the partial sums of max_detections %d x n_hyp %d x %d chunks x 2 channels x chip %d x %d take %zu bytes, more than %llu",
                 max_det, n_hyp, n_chunks, sp->chip_y, sp->chip_x, per_chunk_bytes * n_chunks, (unsigned long long)SARX_TDBP_PAIR_SEARCH_MAX_PARTIAL_BYTES);
        *why = msg;
        return hipErrorInvalidValue;
    }
    TdbpPairSearch* s = nullptr;
    TCK(pair_search_scratch(t, &s));
    cf* rc1 = nullptr;
    TCK(tdbp_pair_rc1(t, &rc1));
    std::vector<PulseGeo> geo;
    tdbp_pulse_table(t, pos, t_pulses, geo);               // position and dt = t_pulse - mean over all n_p
    // window and route: the pair's bounds and the focus's tile condition, evaluated over the whole grid for every hypothesis
    int lo = t->n_s, hi = 0;
    bool series = true, tile = true;
    for (int h = 0; h < n_hyp; ++h) {
        const double* vf = vel_hyps + 3 * h;
        int l = 0, u = t->n_s;
        bool ser = true, til = false;
        tdbp_pair_bounds(t, geo, u0, u1, vf, t_start, scene_size, off_max, a.chirp_centre, &l, &u, &ser, &til);
        if (u > l) { if (l < lo) lo = l; if (u > hi) hi = u; }
        series = series && ser;
        if (tile) tile = til && tdbp_tile_ok(t, geo, vf, scene_size);   // the d_tx series, and the switch SARX_TDBP_TILE=0
    }
    if (t->full_rc) { lo = 0; hi = t->n_s; }
    TCK(tdbp_range_compress(t, raw0, t->rc, lo, hi, st));
    TCK(tdbp_range_compress(t, raw1, rc1, lo, hi, st));
    TCK(tdbp_hyp_upload(s, vel_hyps, n_hyp, st, [&](void* staging) { tdbp_pair_table((PairGeo*)staging, geo, vel, n_p); }));
    TCK(tdbp_ensure_axes(t, scene_size, st));
    TCK(grow(&s->part, &s->part_cap, per_chunk_bytes / sizeof(double2) * n_chunks));
    a.rc[0] = t->rc; a.rc[1] = rc1; a.geo = (const PairGeo*)s->geo; a.xax = t->xax; a.yax = t->yax;
    a.hyps = s->hyps;
    a.rep = d_reports; a.hdr = d_header; a.part = s->part; a.rec = d_records; a.best = d_best; a.chips = d_chips;
    a.nx = t->nx; a.ny = t->ny; a.chip_x = sp->chip_x; a.chip_y = sp->chip_y; a.n_hyp = n_hyp; a.max_det = max_det; a.source = sp->source;
    a.per_chunk = per_chunk; a.chunks = n_chunks;
    const dim3 grid(tiles, max_det * n_hyp, n_chunks);
    if (tile) hipLaunchKernelGGL(tdbp_pair_search_tile_kernel, grid, dim3(256), 0, st, a);
    else if (series) hipLaunchKernelGGL(tdbp_pair_search_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tdbp_pair_search_kernel<false>, grid, dim3(256), 0, st, a);
    TCK(hipGetLastError());
    s->route = tile ? 1 : 0;
    hipLaunchKernelGGL(tdbp_pair_search_metric_kernel, dim3(max_det * n_hyp), dim3(PM), 0, st, a);
    TCK(hipGetLastError());
    hipLaunchKernelGGL(tdbp_pair_search_best_kernel, dim3(max_det), dim3(64), 0, st, a);
    return hipGetLastError();
}

int tdbp_pair_search_route(const Tdbp* t) { return t->pair_search ? t->pair_search->route : -1; }

hipError_t tdbp_pair_search_staging(Tdbp* t, int max_det, const sarx_tdbp_pair_search_params* sp, bool chips, PairSearchStaging* out) {
    TdbpPairSearch* s = nullptr;
    TCK(pair_search_scratch(t, &s));
    const size_t md = (size_t)max_det, n_chip = (size_t)sp->chip_x * sp->chip_y;
    TCK(grow_bytes(&s->raw1, &s->raw1_cap, (size_t)t->n_p * t->n_s * sizeof(float2)));
    TCK(grow_bytes(&s->slot, &s->slot_cap, sizeof(sarx_gmti_header) + md * sizeof(sarx_gmti_report)));
    TCK(grow_bytes(&s->rec, &s->rec_cap, md * sp->n_hyp * sizeof(sarx_tdbp_search_record)));
    TCK(grow_bytes(&s->best, &s->best_cap, md * sizeof(sarx_tdbp_pair_search_best)));
    if (chips) TCK(grow_bytes(&s->chips, &s->chips_cap, md * sp->n_hyp * 2 * n_chip * sizeof(double2)));
    out->raw1 = (float2*)s->raw1; out->slot = s->slot; out->rec = (sarx_tdbp_search_record*)s->rec;
    out->best = (sarx_tdbp_pair_search_best*)s->best; out->chips = chips ? s->chips : nullptr;
    return hipSuccess;
}

}  // namespace sarx
