// Focus-velocity search of the time-domain back-projection: the image of one CPI under n_hyp focus velocities in
// one enqueue, and one 32-byte record of sharpness figures per hypothesis.
//
//   1 range compression, once: tdbp_range_compress over the UNION of the sample windows of all hypotheses (tdbp_sample_window per
//     hypothesis: still a bound, not an estimate).
//   2 back-projection: tdbp_kernel / tdbp_tile_kernel of tdbp.hip with the hypothesis as the grid's third dimension.  The pulse
//     table holds the platform state alone (position, velocity, dt), uploaded once; w = v_plat - v_h and |w|^2 are formed per
//     hypothesis from a device table [n_hyp][3] - per pixel and pulse in the exact form, in the per-(tile, pulse) prologue lane in
//     the tile form, where they cost nothing per pixel.  Everything else - the arithmetic, the float32 interpolation coordinate,
//     the fp64 accumulation - is the code the focus kernels run (tdbp_pixel.hpp), in the same pulse order per pixel.  Partial
//     images [n_hyp][chunks][ny*nx].
//   3 metric launch: one 1024-thread workgroup per hypothesis sums the chunks of every pixel in chunk order, writes the image
//     when a stack is asked for, and folds P = re^2 + im^2 (products and sum rounded one by one, so P is what fp64 NumPy gives)
//     into s2 = sum P, s4 = sum P^2, the peak and its place: thread t takes pixels t, t + 1024, ... in rising order, then a
//     binary tree over the 1024 threads in LDS.  No atomics: the same bits on every run, with or without the stack.
// Pulse chunks: tdbp_pick_chunks (tdbp.hip); pulse and hypothesis tables, their staging and the partial images: a TdbpHypScratch (tdbp_plan.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "tdbp_plan.h"

namespace sarx {

static_assert(sizeof(sarx_tdbp_search_record) == 32, "sarx_tdbp_search_record is 32 bytes");

struct SearchGeo {           // one 64-byte record per pulse: the platform alone, no focus velocity
    double px, py, pz;
    double vx, vy, vz;
    double dt, pad;
};

struct SearchArgs {
    const cf* rc;            // [n_p][n_s]
    const SearchGeo* geo;
    const double* hyps;      // [n_hyp][3]
    const double *xax, *yax;
    double2* part;           // [n_hyp][chunks][ny*nx]
    double inv_c, fc, fs, t_start, k_shift, inv_ns;
    float half_w;
    int n_p, n_s, nx, ny, per_chunk, chunks;
};

__global__ __launch_bounds__(256) void tdbp_search_kernel(SearchArgs a) {
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const double gx0 = a.xax[px.live ? px.ix : 0], gy0 = a.yax[px.live ? px.iy : 0];
    const double vfx = a.hyps[3 * blockIdx.z], vfy = a.hyps[3 * blockIdx.z + 1], vfz = a.hyps[3 * blockIdx.z + 2];
    const int p0 = blockIdx.y * a.per_chunk, p1 = min(a.n_p, p0 + a.per_chunk);
    double acc_re = 0.0, acc_im = 0.0;
    for (int p = p0; p < p1; ++p) {
        const SearchGeo g = a.geo[p];
        const double wx = g.vx - vfx, wy = g.vy - vfy, wz = g.vz - vfz;                     // v_rel (:211) of this hypothesis
        const double w2 = wx * wx + wy * wy + wz * wz;
        const double dx = fma(vfx, g.dt, gx0) - g.px;
        const double dy = fma(vfy, g.dt, gy0) - g.py;
        const double dz = vfz * g.dt - g.pz;
        tdbp_exact_pixel(a, dx, dy, dz, wx, wy, wz, w2, p, acc_re, acc_im);
    }
    const size_t n_pix = (size_t)a.nx * a.ny;
    if (px.live) a.part[((size_t)blockIdx.z * a.chunks + blockIdx.y) * n_pix + (size_t)px.iy * a.nx + px.ix] = make_double2(acc_re, acc_im);
}

// tdbp_tile_kernel with the prologue lane forming w of this hypothesis
__global__ __launch_bounds__(256) void tdbp_search_tile_kernel(SearchArgs a) {
    __shared__ TilePulse s_tp[TP_BATCH];
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const TdbpTileOffsets o = tdbp_tile_offsets(a.xax, a.yax, px, a.nx, a.ny);
    const float qxf = (float)o.qx, qyf = (float)o.qy;
    const double vfx = a.hyps[3 * blockIdx.z], vfy = a.hyps[3 * blockIdx.z + 1], vfz = a.hyps[3 * blockIdx.z + 2];
    const int p0 = blockIdx.y * a.per_chunk, p1 = min(a.n_p, p0 + a.per_chunk);
    const double two_inv_ns = 2.0 * a.inv_ns;
    double acc_re = 0.0, acc_im = 0.0;
    for (int pb = p0; pb < p1; pb += TP_BATCH) {
        const int nb = min(TP_BATCH, p1 - pb);
        __syncthreads();                                   // the previous batch has been consumed
        if ((int)threadIdx.x < nb) {
            const SearchGeo g = a.geo[pb + threadIdx.x];
            const double wx = g.vx - vfx, wy = g.vy - vfy, wz = g.vz - vfz;
            const double w2 = wx * wx + wy * wy + wz * wz;
            const double dx = fma(vfx, g.dt, o.xc) - g.px, dy = fma(vfy, g.dt, o.yc) - g.py, dz = vfz * g.dt - g.pz;
            s_tp[threadIdx.x] = tdbp_tile_prologue(a, dx, dy, dz, wx, wy, wz, w2);
        }
        __syncthreads();
        for (int k = 0; k < nb; ++k) tdbp_tile_pixel(a, s_tp[k], o.qx, o.qy, o.q2, qxf, qyf, two_inv_ns, pb + k, acc_re, acc_im);
    }
    const size_t n_pix = (size_t)a.nx * a.ny;
    if (px.live) a.part[((size_t)blockIdx.z * a.chunks + blockIdx.y) * n_pix + (size_t)px.iy * a.nx + px.ix] = make_double2(acc_re, acc_im);
}

static constexpr int MT = 1024;
static constexpr unsigned long long NO_PIXEL = ~0ull;

// part: [n_hyp][chunks][n_pix]; stack: [n_hyp][n_pix] or NULL; rec: [n_hyp].  One workgroup per hypothesis.
__global__ __launch_bounds__(MT) void tdbp_search_metric_kernel(const double2* part, int chunks, size_t n_pix, int nx, double2* stack,
                                                                sarx_tdbp_search_record* rec) {
    __shared__ double s_s2[MT], s_s4[MT], s_pk[MT];
    __shared__ unsigned long long s_at[MT];
    const int t = threadIdx.x;
    const size_t h = blockIdx.x;
    const double2* src = part + h * (size_t)chunks * n_pix;
    double s2 = 0.0, s4 = 0.0, pk = -1.0;
    unsigned long long at = NO_PIXEL;
    for (size_t i = t; i < n_pix; i += MT) {
        // tdbp_sum_chunks, kept in place: called from here it costs two vector instructions (profiles/r18_tdbp_host_resource_usage.txt)
        double re = 0.0, im = 0.0;
        for (int c = 0; c < chunks; ++c) {
            const double2 v = src[(size_t)c * n_pix + i];
            re += v.x;
            im += v.y;
        }
        if (stack) stack[h * n_pix + i] = make_double2(re, im);
        const double p = __dadd_rn(__dmul_rn(re, re), __dmul_rn(im, im));
        s2 = __dadd_rn(s2, p);
        s4 = __dadd_rn(s4, __dmul_rn(p, p));
        if (p > pk) { pk = p; at = i; }                    // rising i: the first of equal maxima stays
    }
    s_s2[t] = s2; s_s4[t] = s4; s_pk[t] = pk; s_at[t] = at;
    __syncthreads();
    for (int s = MT / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_s2[t] = __dadd_rn(s_s2[t], s_s2[t + s]);
            s_s4[t] = __dadd_rn(s_s4[t], s_s4[t + s]);
            const double o = s_pk[t + s];
            const unsigned long long oa = s_at[t + s];
            if (o > s_pk[t] || (o == s_pk[t] && oa < s_at[t])) { s_pk[t] = o; s_at[t] = oa; }
        }
        __syncthreads();
    }
    if (t == 0) {
        sarx_tdbp_search_record r;
        r.s2 = s_s2[0]; r.s4 = s_s4[0];
        if (s_at[0] == NO_PIXEL) {                         // no pixel compared greater than -1: every power is NaN
            r.peak = s_s2[0]; r.peak_ix = -1; r.peak_iy = -1;
        } else {
            r.peak = s_pk[0];
            r.peak_ix = (int32_t)(s_at[0] % (unsigned long long)nx);
            r.peak_iy = (int32_t)(s_at[0] / (unsigned long long)nx);
        }
        rec[h] = r;
    }
}

struct TdbpSearch : TdbpHypScratch {                       // the table holds SearchGeo
    sarx_tdbp_search_record* rec = nullptr;                // staging of the host entry point
    double2* stack = nullptr;
    size_t stack_cap = 0;
};

void tdbp_search_free(TdbpSearch* s) {
    if (!s) return;
    tdbp_hyp_scratch_free(s);
    hipFree(s->rec); hipFree(s->stack);
    delete s;
}

static hipError_t search_scratch(Tdbp* t, TdbpSearch** out) {
    if (!t->search) {
        TdbpSearch* s = new TdbpSearch();
        const hipError_t e = tdbp_hyp_scratch_init(s, t->n_p, sizeof(SearchGeo), SARX_TDBP_SEARCH_MAX_HYP);
        if (e != hipSuccess) { tdbp_search_free(s); return e; }
        t->search = s;
    }
    *out = t->search;
    return hipSuccess;
}

static hipError_t launch_metric(const Tdbp* t, const double2* part, int chunks, int n_hyp, double2* d_images,
                                sarx_tdbp_search_record* d_records, hipStream_t st) {
    hipLaunchKernelGGL(tdbp_search_metric_kernel, dim3(n_hyp), dim3(MT), 0, st, part, chunks, (size_t)t->nx * t->ny, t->nx, d_images, d_records);
    return hipGetLastError();
}

hipError_t tdbp_search(Tdbp* t, const float2* raw, const double* pos, const double* vel, const double* t_pulses, double t_start,
                       const double* vel_hyps, int n_hyp, double scene_size, int chunks, double2* d_images,
                       sarx_tdbp_search_record* d_records, hipStream_t st) {
    TdbpSearch* s = nullptr;
    TCK(search_scratch(t, &s));
    const int n_p = t->n_p;
    // window and route: the bound and the tile condition of the focus, evaluated for every hypothesis
    std::vector<PulseGeo> geo;
    tdbp_pulse_table(t, pos, t_pulses, geo);
    int lo = t->n_s, hi = 0;
    bool tile = true;
    for (int h = 0; h < n_hyp; ++h) {
        const double* vf = vel_hyps + 3 * h;
        tdbp_set_focus(geo, vel, vf);
        int l = 0, u = t->n_s;
        if (!t->full_rc) tdbp_sample_window(t, geo, vf, t_start, scene_size, &l, &u);
        if (u > l) { if (l < lo) lo = l; if (u > hi) hi = u; }
        if (tile) tile = tdbp_tile_ok(t, geo, vf, scene_size);
    }
    TCK(tdbp_range_compress(t, raw, t->rc, lo, hi, st));
    TCK(tdbp_hyp_upload(s, vel_hyps, n_hyp, st, [&](void* staging) {
        SearchGeo* h_geo = (SearchGeo*)staging;
        for (int p = 0; p < n_p; ++p) {
            SearchGeo& g = h_geo[p];
            g.px = geo[p].px; g.py = geo[p].py; g.pz = geo[p].pz;
            g.vx = vel[3 * p]; g.vy = vel[3 * p + 1]; g.vz = vel[3 * p + 2];
            g.dt = geo[p].dt; g.pad = 0.0;
        }
    }));
    TCK(tdbp_ensure_axes(t, scene_size, st));
    // a chunk launches tiles x n_hyp workgroups: fewer chunks with more hypotheses, the partial images stay near 16384 workgroups x 4 KiB
    const int tiles = ((t->nx + 15) / 16) * ((t->ny + 15) / 16);
    int per_chunk = 0;
    chunks = tdbp_pick_chunks(tiles, n_hyp, n_p, chunks, &per_chunk);
    TCK(grow(&s->part, &s->part_cap, (size_t)n_hyp * chunks * t->nx * t->ny));
    SearchArgs a{};
    tdbp_fill_args(t, t_start, per_chunk, a);
    a.geo = (const SearchGeo*)s->geo; a.hyps = s->hyps; a.part = s->part; a.chunks = chunks;
    const dim3 grid(tiles, chunks, n_hyp);
    if (tile) hipLaunchKernelGGL(tdbp_search_tile_kernel, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tdbp_search_kernel, grid, dim3(256), 0, st, a);
    TCK(hipGetLastError());
    s->route = tile ? 1 : 0;
    return launch_metric(t, s->part, chunks, n_hyp, d_images, d_records, st);
}

hipError_t tdbp_search_metric(Tdbp* t, const double2* d_stack, int n_hyp, sarx_tdbp_search_record* d_records, hipStream_t st) {
    return launch_metric(t, d_stack, 1, n_hyp, nullptr, d_records, st);
}

int tdbp_search_route(const Tdbp* t) { return t->search ? t->search->route : -1; }

hipError_t tdbp_search_staging(Tdbp* t, int n_hyp, bool images, sarx_tdbp_search_record** d_records, double2** d_images, hipStream_t st) {
    TdbpSearch* s = nullptr;
    TCK(search_scratch(t, &s));
    if (!s->rec) TCK(hipMalloc(&s->rec, (size_t)SARX_TDBP_SEARCH_MAX_HYP * sizeof(sarx_tdbp_search_record)));
    *d_records = s->rec;
    *d_images = nullptr;
    if (images) {
        TCK(grow(&s->stack, &s->stack_cap, (size_t)n_hyp * t->nx * t->ny));
        *d_images = s->stack;
    }
    return hipSuccess;
}

}  // namespace sarx
