// Two-receiver back-projection: both receive channels of the two-receiver echo model
// (sar_ati_dcpa_sim_csa.py:113-178) imaged onto one ground grid in one enqueue.
//
//   1 range compression, once per channel: tdbp_range_compress over ONE sample window that bounds what either channel can touch
//     (pair_bounds, on the focus's moved_rect_range and tdbp_clamp_window: a bound, not an estimate).  Channel 0 lands in the
//     plan's rc buffer, channel 1 in the scratch's: tdbp_range_compress takes its destination.
//   2 back-projection: one thread per pixel carries BOTH channels.  Per pulse the pixel moved with the focus velocity, the
//     vector to the transmitter, d_tx and its reciprocal square root and d . v^ are computed once; each channel adds only its
//     receive leg (tdbp_pair_pixel of tdbp_pixel.hpp), the float32 interpolation coordinate and its sample (tdbp_sample).  The
//     loop runs over the UNION of the two channels' pulse ranges; a channel accumulates only inside its own range (a
//     wave-uniform test).  Pulses split into chunks across blockIdx.y, partial images [2][chunks][ny*nx].
//   3 reduce launch: the chunks of every pixel summed in chunk order, written as complex128 and / or as complex64 (the fp64 sum
//     rounded once).  No atomics: the same bits on every run.
// Two forms of the geometry, as in tdbp.hip: the exact one (tdbp_pair_kernel), and the one expanded about the reference pixel of each
// 16 x 16 tile (tdbp_pair_tile_kernel: one lane per pulse fills a 256-pulse batch of records in LDS, every pixel walks them), taken
// when tdbp_tile_ok and pair_tile_ok bound its truncation error below 1e-9 m for both channels.  Same pulse order per pixel, same
// fp64 accumulation.  Both pulse loops are tdbp_pixel.hpp's (tdbp_pair_pulses, tdbp_pair_tile_pulses): the search on the pair
// (tdbp_pair_search.hip) runs them too.  Pulse chunks: tdbp_pick_chunks (tdbp.hip); pulse table, staging and partial images: a TdbpScratch (tdbp_plan.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "tdbp_plan.h"

namespace sarx {

static_assert(sizeof(sarx_tdbp_pair_params) == 40, "sarx_tdbp_pair_params is 40 bytes");

struct PairArgs {
    PairChan ch[2];
    const PairGeo* geo;
    const double *xax, *yax;
    double2* part;           // [2][chunks][ny*nx]
    double vfx, vfy, vfz;
    double off[2];
    double inv_c, fs, t_start, chirp_centre, inv_ns;
    int first[2], n_used;    // channel c: pulses [first[c], first[c] + n_used)
    int u0, u1;              // their union
    int nx, ny, per_chunk, chunks;
};

// the partial images of both channels for this workgroup's chunk = blockIdx.y
__device__ __forceinline__ void store_partial(const PairArgs& a, const TdbpPix& px, double re0, double im0, double re1, double im1) {
    if (!px.live) return;
    const size_t n_pix = (size_t)a.nx * a.ny, at = (size_t)blockIdx.y * n_pix + (size_t)px.iy * a.nx + px.ix;
    a.part[at] = make_double2(re0, im0);
    a.part[(size_t)a.chunks * n_pix + at] = make_double2(re1, im1);
}

template <bool SERIES> __global__ __launch_bounds__(256) void tdbp_pair_kernel(PairArgs a) {
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const double gx0 = a.xax[px.live ? px.ix : 0], gy0 = a.yax[px.live ? px.iy : 0];
    const int p0 = a.u0 + blockIdx.y * a.per_chunk, p1 = min(a.u1, p0 + a.per_chunk);
    double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
    tdbp_pair_pulses<SERIES>(a, a.vfx, a.vfy, a.vfz, gx0, gy0, p0, p1, re0, im0, re1, im1);
    store_partial(a, px, re0, im0, re1, im1);
}

// the tile form (tdbp_pixel.hpp): one lane per pulse fills the batch's records, then every pixel walks them
__global__ __launch_bounds__(256) void tdbp_pair_tile_kernel(PairArgs a) {
    __shared__ PairTilePulse s_tp[TP_BATCH];
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const TdbpTileOffsets o = tdbp_tile_offsets(a.xax, a.yax, px, a.nx, a.ny);
    const int p0 = a.u0 + blockIdx.y * a.per_chunk, p1 = min(a.u1, p0 + a.per_chunk);
    double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
    tdbp_pair_tile_pulses(a, s_tp, a.vfx, a.vfy, a.vfz, o, p0, p1, re0, im0, re1, im1);
    store_partial(a, px, re0, im0, re1, im1);
}

// part: [2][chunks][n_pix]; out128: [2][n_pix] or NULL; out64: [2][n_pix] or NULL
__global__ __launch_bounds__(256) void tdbp_pair_reduce_kernel(const double2* part, int chunks, size_t n_pix, double2* out128, float2* out64) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pix) return;
    for (int ch = 0; ch < 2; ++ch) {
        const double2 z = tdbp_sum_chunks(part + (size_t)ch * chunks * n_pix, chunks, n_pix, i);
        if (out128) out128[(size_t)ch * n_pix + i] = z;
        if (out64) out64[(size_t)ch * n_pix + i] = make_float2((float)z.x, (float)z.y);
    }
}

struct TdbpPair : TdbpScratch {                            // the table holds PairGeo
    cf* rc1 = nullptr;                                     // [n_p][n_s] range-compressed pulses of channel 1
    float2* raw1 = nullptr;                                // staging of the host entry point
    double2* img128 = nullptr;
    float2* img64 = nullptr;
};

void tdbp_pair_free(TdbpPair* s) {
    if (!s) return;
    tdbp_scratch_free(s);
    hipFree(s->rc1); hipFree(s->raw1); hipFree(s->img128); hipFree(s->img64);
    delete s;
}

static hipError_t pair_scratch(Tdbp* t, TdbpPair** out) {
    if (!t->pair) {
        TdbpPair* s = new TdbpPair();
        hipError_t e = tdbp_scratch_init(s, t->n_p, sizeof(PairGeo));
        if (e == hipSuccess) e = hipMalloc(&s->rc1, (size_t)t->n_p * t->n_s * sizeof(cf));
        if (e != hipSuccess) { tdbp_pair_free(s); return e; }
        t->pair = s;
    }
    *out = t->pair;
    return hipSuccess;
}

// Sample window [lo, hi) that either channel can touch over the pulses [u0, u1), whether the series of tdbp_pair_pixel holds, and
// whether the pair's part of the tile expansion does (the d_tx part is tdbp_tile_ok's).
// d_tx lies in moved_rect_range (tdbp.hip); the receiver is |off| from the transmitter, so |d_rx - d_tx| <= |off| (triangle inequality) and
// |e| = |d_rx^2 / d_tx^2 - 1| <= 2 |off| / d_tx + (off / d_tx)^2.
void tdbp_pair_bounds(const Tdbp* t, const std::vector<PulseGeo>& geo, int u0, int u1, const double* vf, double t_start, double scene_size,
                      const sarx_tdbp_pair_params* prm, int* lo, int* hi, bool* series, bool* tile) {
    const double c = t->k.c, fs = t->k.fs, h = scene_size / 2;
    const double om = fmax(fabs(prm->rx_offset_m[0]), fabs(prm->rx_offset_m[1]));
    double imin = 1e300, imax = -1e300;
    *series = true;
    // the remainder of d_tx - d_rx about a tile's reference pixel (tdbp_pixel.hpp): |q|^2 |off| / (sqrt(3) (d_min - |off|)^2), q the
    // tile's reach (tdbp_tile_reach), as tdbp_tile_ok takes it
    const double qm = tdbp_tile_reach(t, scene_size);
    *tile = qm >= 0.0;
    for (int p = u0; p < u1; ++p) {
        double dmin, dmax;
        moved_rect_range(geo[p], vf, h, &dmin, &dmax);
        const double a = ((2.0 * dmin - om) / c - t_start + prm->chirp_centre_s) * fs;
        const double b = ((2.0 * dmax + om) / c - t_start + prm->chirp_centre_s) * fs;
        if (a < imin) imin = a;
        if (b > imax) imax = b;
        const double e = 2.0 * om / dmin + (om / dmin) * (om / dmin);
        if (!(dmin > 0.0) || !(7.0 / 256.0 * e * e * e * e * e * dmax < 1e-9)) *series = false;
        if (!(dmin > om) || !(qm * qm * om / (sqrt(3.0) * (dmin - om) * (dmin - om)) < 1e-9)) *tile = false;
    }
    tdbp_clamp_window(imin, imax, t->n_s, lo, hi);
}

void tdbp_pair_table(PairGeo* h_geo, const std::vector<PulseGeo>& geo, const double* vel, int n_p) {
    for (int p = 0; p < n_p; ++p) {
        PairGeo& g = h_geo[p];
        const double vx = vel[3 * p], vy = vel[3 * p + 1], vz = vel[3 * p + 2];
        const double inv = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
        g.px = geo[p].px; g.py = geo[p].py; g.pz = geo[p].pz;
        g.ux = vx * inv; g.uy = vy * inv; g.uz = vz * inv;
        g.dt = geo[p].dt; g.pad = 0.0;
    }
}

hipError_t tdbp_pair_rc1(Tdbp* t, cf** rc1) {
    TdbpPair* s = nullptr;
    TCK(pair_scratch(t, &s));
    *rc1 = s->rc1;
    return hipSuccess;
}

hipError_t tdbp_pair(Tdbp* t, const float2* raw0, const float2* raw1, const double* pos, const double* vel, const double* t_pulses,
                     double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_pair_params* prm, int chunks,
                     double2* d_img128, float2* d_img64, hipStream_t st) {
    TdbpPair* s = nullptr;
    TCK(pair_scratch(t, &s));
    const int n_p = t->n_p;
    int u0 = 0, u1 = 0;
    tdbp_pair_union(prm, &u0, &u1);
    std::vector<PulseGeo> geo;
    tdbp_pulse_table(t, pos, t_pulses, geo);               // position and dt = t_pulse - mean over all n_p
    int lo = 0, hi = t->n_s;
    bool series = true, tile = false;
    tdbp_pair_bounds(t, geo, u0, u1, vel_focus, t_start, scene_size, prm, &lo, &hi, &series, &tile);
    tile = tile && tdbp_tile_ok(t, geo, vel_focus, scene_size);   // the d_tx series, and the switch SARX_TDBP_TILE=0
    if (t->full_rc) { lo = 0; hi = t->n_s; }
    TCK(tdbp_range_compress(t, raw0, t->rc, lo, hi, st));
    TCK(tdbp_range_compress(t, raw1, s->rc1, lo, hi, st)); // the same launches, the other destination
    TCK(tdbp_scratch_upload(s, st, [&](void* staging) {
        tdbp_pair_table((PairGeo*)staging, geo, vel, n_p);
        return hipSuccess;
    }));
    TCK(tdbp_ensure_axes(t, scene_size, st));
    // pulse chunks over the union's pulses, one chunk launching tiles workgroups
    const int tiles = ((t->nx + 15) / 16) * ((t->ny + 15) / 16);
    int per_chunk = 0;
    chunks = tdbp_pick_chunks(tiles, 1, u1 - u0, chunks, &per_chunk);
    const size_t n_pix = (size_t)t->nx * t->ny;
    TCK(grow(&s->part, &s->part_cap, 2 * (size_t)chunks * n_pix));
    PairArgs a{};
    tdbp_pair_fill_args(t, s, s->rc1, t_start, prm, a);
    a.part = s->part;
    a.vfx = vel_focus[0]; a.vfy = vel_focus[1]; a.vfz = vel_focus[2];
    a.nx = t->nx; a.ny = t->ny; a.per_chunk = per_chunk; a.chunks = chunks;
    if (tile) hipLaunchKernelGGL(tdbp_pair_tile_kernel, dim3(tiles, chunks), dim3(256), 0, st, a);
    else if (series) hipLaunchKernelGGL(tdbp_pair_kernel<true>, dim3(tiles, chunks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tdbp_pair_kernel<false>, dim3(tiles, chunks), dim3(256), 0, st, a);
    TCK(hipGetLastError());
    s->route = tile ? 1 : 0;
    hipLaunchKernelGGL(tdbp_pair_reduce_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st, s->part, chunks, n_pix, d_img128, d_img64);
    return hipGetLastError();
}

int tdbp_pair_route(const Tdbp* t) { return t->pair ? t->pair->route : -1; }

hipError_t tdbp_pair_staging(Tdbp* t, float2** d_raw1, double2** d_img128, float2** d_img64) {
    TdbpPair* s = nullptr;
    TCK(pair_scratch(t, &s));
    const size_t n_pix = (size_t)t->nx * t->ny;
    if (!s->raw1) TCK(hipMalloc(&s->raw1, (size_t)t->n_p * t->n_s * sizeof(float2)));
    if (!s->img128) TCK(hipMalloc(&s->img128, 2 * n_pix * sizeof(double2)));
    if (!s->img64) TCK(hipMalloc(&s->img64, 2 * n_pix * sizeof(float2)));
    *d_raw1 = s->raw1; *d_img128 = s->img128; *d_img64 = s->img64;
    return hipSuccess;
}

}  // namespace sarx
