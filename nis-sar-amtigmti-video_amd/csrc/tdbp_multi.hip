// N-receiver back-projection and the multi-baseline ATI resolver (include/sarx_tdbp_multi.h).
//
// The stack: n_rx = 2, 3 or 4 receive channels imaged onto one ground grid in one enqueue.  The two-receiver pair (tdbp_pair.hip,
// DESIGN.md 4.18) is its n_rx = 2 case on a scratch of its own:
//   1 range compression, once per channel, over ONE sample window that bounds what any channel can touch (tdbp_pair_bounds with the
//     largest |offset|: a bound, not an estimate).  Channel 0 lands in the plan's rc buffer, channels 1 .. 3 in the scratch's:
//     tdbp_range_compress takes its destination.
//   2 back-projection: one thread per pixel carries all N channels.  Per pulse the pixel moved with the focus velocity, the vector to
//     the transmitter, d_tx, its reciprocal square root and d . v^ are computed once; each channel adds only its receive leg, its
//     interpolation coordinate and its sample.  The loop runs over the UNION of the channels' pulse ranges; a channel accumulates only
//     inside its own range (a wave-uniform test).  Pulses split into chunks across blockIdx.y, partial images [n_rx][chunks][ny*nx].
//   3 one reduce launch over the N channels: chunks summed in chunk order, written as complex128 and / or complex64.  No atomics.
// Two forms of the geometry, templated on N: the exact one (tdbp_multi_kernel<N, SERIES>) and the tile-expanded one
// (tdbp_multi_tile_kernel<N>: a 256-pulse batch of 32 + 24 N byte records in LDS, 20, 28 and 32 KiB), taken when tdbp_tile_ok and
// the receivers' bound with the largest |offset| hold.  Same pulse order per pixel, same fp64 accumulation.  The pulse loops are
// tdbp_pixel.hpp's (tdbp_multi_pulses, tdbp_multi_tile_pulses): the search on the pair (tdbp_pair_search.hip) runs them at N = 2.
// Pulse chunks: tdbp_pick_chunks (tdbp.hip); pulse table, channel buffers, staging and partial images: a TdbpRx (tdbp_plan.h).
//
// The resolver (tdbp_multi_resolve_kernel): one lane per report of a GMTI slot, the count read from the slot's header on the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "tdbp_plan.h"

namespace sarx {

static_assert(sizeof(sarx_tdbp_multi_params) == 64, "sarx_tdbp_multi_params is 64 bytes");
static_assert(sizeof(sarx_tdbp_multi_resolve_params) == 56, "sarx_tdbp_multi_resolve_params is 56 bytes");
static_assert(sizeof(sarx_tdbp_multi_record) == 64, "sarx_tdbp_multi_record is 64 bytes");
static_assert(MAX_RX == SARX_TDBP_MULTI_MAX_RX, "RxArgs holds SARX_TDBP_MULTI_MAX_RX channels");

struct MultiArgs : RxArgs {
    const double *xax, *yax;
    double2* part;           // [n_rx][chunks][ny*nx]
    double vfx, vfy, vfz;
    int nx, ny, per_chunk, chunks;
};

// the partial images of all channels for this workgroup's chunk = blockIdx.y
template <int N> __device__ __forceinline__ void store_partial(const MultiArgs& a, const TdbpPix& px, const double (&re)[N], const double (&im)[N]) {
    if (!px.live) return;
    const size_t n_pix = (size_t)a.nx * a.ny, at = (size_t)blockIdx.y * n_pix + (size_t)px.iy * a.nx + px.ix;
#pragma unroll
    for (int c = 0; c < N; ++c) a.part[(size_t)c * a.chunks * n_pix + at] = make_double2(re[c], im[c]);
}

template <int N, bool SERIES> __global__ __launch_bounds__(256) void tdbp_multi_kernel(MultiArgs a) {
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const double gx0 = a.xax[px.live ? px.ix : 0], gy0 = a.yax[px.live ? px.iy : 0];
    const int p0 = a.u0 + blockIdx.y * a.per_chunk, p1 = min(a.u1, p0 + a.per_chunk);
    double re[N] = {}, im[N] = {};
    tdbp_multi_pulses<N, SERIES>(a, a.vfx, a.vfy, a.vfz, gx0, gy0, p0, p1, re, im);
    store_partial<N>(a, px, re, im);
}

// the tile form (tdbp_pixel.hpp): one lane per pulse fills the batch's records, then every pixel walks them
template <int N> __global__ __launch_bounds__(256) void tdbp_multi_tile_kernel(MultiArgs a) {
    __shared__ MultiTilePulse<N> s_tp[TP_BATCH];
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const TdbpTileOffsets o = tdbp_tile_offsets(a.xax, a.yax, px, a.nx, a.ny);
    const int p0 = a.u0 + blockIdx.y * a.per_chunk, p1 = min(a.u1, p0 + a.per_chunk);
    double re[N] = {}, im[N] = {};
    tdbp_multi_tile_pulses<N>(a, s_tp, a.vfx, a.vfy, a.vfz, o, p0, p1, re, im);
    store_partial<N>(a, px, re, im);
}

// part: [n_rx][chunks][n_pix]; out128: [n_rx][n_pix] or NULL; out64: [n_rx][n_pix] or NULL
__global__ __launch_bounds__(256) void tdbp_multi_reduce_kernel(const double2* part, int chunks, size_t n_pix, int n_rx, double2* out128, float2* out64) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pix) return;
    for (int ch = 0; ch < n_rx; ++ch) {
        const double2 z = tdbp_sum_chunks(part + (size_t)ch * chunks * n_pix, chunks, n_pix, i);
        if (out128) out128[(size_t)ch * n_pix + i] = z;
        if (out64) out64[(size_t)ch * n_pix + i] = make_float2((float)z.x, (float)z.y);
    }
}

void tdbp_rx_free(TdbpRx* s) {
    if (!s) return;
    tdbp_scratch_free(s);
    for (int c = 0; c < MAX_RX - 1; ++c) { hipFree(s->rc[c]); hipFree(s->raw[c]); }
    hipFree(s->img128); hipFree(s->img64);
    delete s;
}

hipError_t tdbp_rx_scratch(Tdbp* t, TdbpRx*& inst, int cap, int n_rx, TdbpRx** out) {
    if (!inst) {
        TdbpRx* s = new TdbpRx();
        s->cap = cap;
        const hipError_t e = tdbp_scratch_init(s, t->n_p, sizeof(PairGeo));
        if (e != hipSuccess) { tdbp_rx_free(s); return e; }
        inst = s;
    }
    for (int c = 0; c < n_rx - 1; ++c)
        if (!inst->rc[c]) TCK(hipMalloc(&inst->rc[c], (size_t)t->n_p * t->n_s * sizeof(cf)));
    *out = inst;
    return hipSuccess;
}

template <int N> static void launch_multi(const MultiArgs& a, bool tile, bool series, dim3 grid, hipStream_t st) {
    if (tile) hipLaunchKernelGGL(tdbp_multi_tile_kernel<N>, grid, dim3(256), 0, st, a);
    else if (series) hipLaunchKernelGGL((tdbp_multi_kernel<N, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((tdbp_multi_kernel<N, false>), grid, dim3(256), 0, st, a);
}

hipError_t tdbp_rx(Tdbp* t, TdbpRx*& inst, int cap, const float2* const* raw, const double* pos, const double* vel, const double* t_pulses,
                   double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* prm, int chunks,
                   double2* d_img128, float2* d_img64, hipStream_t st) {
    const int n_rx = prm->n_rx, n_p = t->n_p;
    TdbpRx* s = nullptr;
    TCK(tdbp_rx_scratch(t, inst, cap, n_rx, &s));
    MultiArgs a{};
    tdbp_rx_fill_args(t, t_start, prm, a);
    std::vector<PulseGeo> geo;
    tdbp_pulse_table(t, pos, t_pulses, geo);               // position and dt = t_pulse - mean over all n_p
    int lo = 0, hi = t->n_s;
    bool series = true, tile = false;
    tdbp_pair_bounds(t, geo, a.u0, a.u1, vel_focus, t_start, scene_size, tdbp_rx_off_max(a, n_rx), a.chirp_centre, &lo, &hi, &series, &tile);
    tile = tile && tdbp_tile_ok(t, geo, vel_focus, scene_size);   // the d_tx series, and the switch SARX_TDBP_TILE=0
    if (t->full_rc) { lo = 0; hi = t->n_s; }
    for (int c = 0; c < n_rx; ++c) {
        cf* const dst = c ? s->rc[c - 1] : t->rc;          // the same launches, the channel's destination
        a.rc[c] = dst;
        TCK(tdbp_range_compress(t, raw[c], dst, lo, hi, st));
    }
    TCK(tdbp_scratch_upload(s, st, [&](void* staging) {
        tdbp_pair_table((PairGeo*)staging, geo, vel, n_p);
        return hipSuccess;
    }));
    TCK(tdbp_ensure_axes(t, scene_size, st));
    // pulse chunks over the union's pulses, one chunk launching tiles workgroups
    const int tiles = ((t->nx + 15) / 16) * ((t->ny + 15) / 16);
    int per_chunk = 0;
    chunks = tdbp_pick_chunks(tiles, 1, a.u1 - a.u0, chunks, &per_chunk);
    const size_t n_pix = (size_t)t->nx * t->ny;
    TCK(grow(&s->part, &s->part_cap, (size_t)n_rx * chunks * n_pix));
    a.geo = (const PairGeo*)s->geo; a.xax = t->xax; a.yax = t->yax;
    a.part = s->part;
    a.vfx = vel_focus[0]; a.vfy = vel_focus[1]; a.vfz = vel_focus[2];
    a.nx = t->nx; a.ny = t->ny; a.per_chunk = per_chunk; a.chunks = chunks;
    const dim3 grid(tiles, chunks);
    if (n_rx == 2) launch_multi<2>(a, tile, series, grid, st);
    else if (n_rx == 3) launch_multi<3>(a, tile, series, grid, st);
    else launch_multi<4>(a, tile, series, grid, st);
    TCK(hipGetLastError());
    s->route = tile ? 1 : 0;
    hipLaunchKernelGGL(tdbp_multi_reduce_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st, s->part, chunks, n_pix, n_rx, d_img128, d_img64);
    return hipGetLastError();
}

hipError_t tdbp_multi(Tdbp* t, const float2* const* raw, const double* pos, const double* vel, const double* t_pulses, double t_start,
                      const double* vel_focus, double scene_size, const sarx_tdbp_multi_params* prm, int chunks, double2* d_img128,
                      float2* d_img64, hipStream_t st) {
    return tdbp_rx(t, t->multi, MAX_RX, raw, pos, vel, t_pulses, t_start, vel_focus, scene_size, prm, chunks, d_img128, d_img64, st);
}

int tdbp_multi_route(const Tdbp* t) { return t->multi ? t->multi->route : -1; }

void tdbp_rx_held(const Tdbp* t, const TdbpRx* s, uint64_t* bytes, uint64_t* id) {
    *bytes = 0; *id = 0;
    if (!s) return;
    const size_t n = (size_t)t->n_p * t->n_s, n_pix = (size_t)t->nx * t->ny;
    const auto held = [&](const void* p, size_t b) { if (p) { *bytes += b; *id += (uint64_t)(uintptr_t)p; } };
    held(s->geo, s->bytes);
    held(s->part, s->part_cap * sizeof(double2));
    for (int c = 0; c < MAX_RX - 1; ++c) { held(s->rc[c], n * sizeof(cf)); held(s->raw[c], n * sizeof(float2)); }
    held(s->img128, s->cap * n_pix * sizeof(double2));
    held(s->img64, s->cap * n_pix * sizeof(float2));
}

void tdbp_multi_held(const Tdbp* t, uint64_t* bytes, uint64_t* id) { tdbp_rx_held(t, t->multi, bytes, id); }

hipError_t tdbp_rx_staging(Tdbp* t, TdbpRx*& inst, int cap, int n_rx, float2** d_raw, double2** d_img128, float2** d_img64) {
    TdbpRx* s = nullptr;
    TCK(tdbp_rx_scratch(t, inst, cap, n_rx, &s));
    const size_t n_pix = (size_t)t->nx * t->ny;
    for (int c = 0; c < n_rx - 1; ++c) {
        if (!s->raw[c]) TCK(hipMalloc(&s->raw[c], (size_t)t->n_p * t->n_s * sizeof(float2)));
        d_raw[c] = s->raw[c];
    }
    if (!s->img128) TCK(hipMalloc(&s->img128, s->cap * n_pix * sizeof(double2)));
    if (!s->img64) TCK(hipMalloc(&s->img64, s->cap * n_pix * sizeof(float2)));
    *d_img128 = s->img128; *d_img64 = s->img64;
    return hipSuccess;
}

hipError_t tdbp_multi_staging(Tdbp* t, int n_rx, float2** d_raw, double2** d_img128, float2** d_img64) {
    return tdbp_rx_staging(t, t->multi, MAX_RX, n_rx, d_raw, d_img128, d_img64);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The resolver: include/sarx_tdbp_multi.h, part 2, statement for statement.  One lane per report; a report's three sums, its wrap
// search (at most SARX_TDBP_MULTI_MAX_CANDIDATES + 2 steps) and its record are the lane's own, so nothing is shared and the
// records are the same bytes on every run.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pick3(const double (&v)[3], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : v[2]; }

__global__ __launch_bounds__(256) void tdbp_multi_resolve_kernel(MultiResolveArgs a) {
    constexpr double PI = 3.14159265358979323846, TWO_PI = 2.0 * PI, FOUR_PI = 4.0 * PI;
    const sarx_gmti_header h = *(const sarx_gmti_header*)a.slot;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    sarx_tdbp_multi_record out;
    out.v_los = out.v_coarse = out.cost = out.cost_next = 0.0;
    out.phase[0] = out.phase[1] = out.phase[2] = 0.0;
    out.k = 0;
    out.status = SARX_TDBP_MULTI_OK;
    if (h.overflow != 0 || h.count > (uint32_t)a.p.max_detections) {   // never a truncated answer
        out.status = SARX_TDBP_MULTI_OVERFLOW;
        if (r == 0) a.rec[0] = out;
        return;
    }
    if (r >= h.count) return;
    const sarx_gmti_report rep = ((const sarx_gmti_report*)(a.slot + sizeof(sarx_gmti_header)))[r];
    const int nb = a.p.n_rx - 1;
    const long long i0 = max((long long)rep.i - a.p.half, 0LL), i1 = min((long long)rep.i + a.p.half, (long long)a.ny - 1);
    const long long j0 = max((long long)rep.j - a.p.half, 0LL), j1 = min((long long)rep.j + a.p.half, (long long)a.nx - 1);
    const size_t n_pix = (size_t)a.ny * a.nx;
    double wre[3] = {0.0, 0.0, 0.0}, wim[3] = {0.0, 0.0, 0.0};
    for (long long i = i0; i <= i1; ++i)
        for (long long j = j0; j <= j1; ++j) {
            const size_t at = (size_t)i * a.nx + (size_t)j;
            const float2 z0 = a.imgs[at];
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < nb) {
                    const float2 z = a.imgs[(size_t)(b + 1) * n_pix + at];
                    const double tr = (double)z0.x * (double)z.x + (double)z0.y * (double)z.y;   // exact products, one rounding
                    const double ti = (double)z0.y * (double)z.x - (double)z0.x * (double)z.y;
                    wre[b] += tr;
                    wim[b] += ti;
                }
        }
    const double lag[3] = {a.p.lag_s[0], a.p.lag_s[1], a.p.lag_s[2]};
    double phi[3] = {0.0, 0.0, 0.0};
    bool zero = false;
    int B = 0, S = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b)
        if (b < nb) {
            phi[b] = atan2(wim[b], wre[b]);
            zero = zero || (wre[b] == 0.0 && wim[b] == 0.0);
            if (fabs(lag[b]) > fabs(pick3(lag, B))) B = b;
            if (fabs(lag[b]) < fabs(pick3(lag, S))) S = b;
        }
    out.phase[0] = phi[0]; out.phase[1] = phi[1]; out.phase[2] = phi[2];
    if (zero) {
        out.status = SARX_TDBP_MULTI_ZERO;
        a.rec[r] = out;
        return;
    }
    const double lam = a.p.wavelength_m, v_max = a.p.v_max_mps;
    const double phi_b = pick3(phi, B), lag_b = pick3(lag, B);
    out.v_coarse = -lam * pick3(phi, S) / (FOUR_PI * pick3(lag, S));
    // every k with |v_k| <= v_max lies in [(-x - phi_B) / 2 pi, (x - phi_B) / 2 pi], x = 4 pi |lag_B| v_max / lambda; one more at either
    // end against the rounding of the ends, the test itself is the header's
    const double x = FOUR_PI * fabs(lag_b) * v_max / lam;
    const int k_lo = (int)ceil((-x - phi_b) / TWO_PI) - 1, k_hi = (int)floor((x - phi_b) / TWO_PI) + 1;
    bool any = false;
    int k_best = 0;
    double j_best = 0.0, j_next = INFINITY, v_best = 0.0;
    for (int k = k_lo; k <= k_hi; ++k) {
        const double v = -lam * (phi_b + TWO_PI * (double)k) / (FOUR_PI * lag_b);
        if (!(fabs(v) <= v_max)) continue;
        double cost = 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (b < nb && b != B) {
                const double y = phi[b] + FOUR_PI * lag[b] * v / lam;
                const double w = y - TWO_PI * ceil((y - PI) / TWO_PI);
                cost += w * w;
            }
        const bool better = !any || cost < j_best ||
                            (cost == j_best && (abs(k) < abs(k_best) || (abs(k) == abs(k_best) && k > k_best)));
        if (better) {
            if (any) j_next = fmin(j_next, j_best);
            j_best = cost; k_best = k; v_best = v; any = true;
        } else {
            j_next = fmin(j_next, cost);
        }
    }
    if (!any) {
        out.status = SARX_TDBP_MULTI_NO_CANDIDATE;
        out.cost = out.cost_next = INFINITY;
    } else {
        out.v_los = v_best; out.k = k_best; out.cost = j_best; out.cost_next = j_next;
    }
    a.rec[r] = out;
}

hipError_t launch_multi_resolve(const MultiResolveArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(tdbp_multi_resolve_kernel, dim3((unsigned)((a.p.max_detections + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sarx
