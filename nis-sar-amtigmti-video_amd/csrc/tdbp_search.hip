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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
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
    const int tiles_x = (a.nx + 15) >> 4;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int ix = tx * 16 + (threadIdx.x & 15), iy = ty * 16 + (threadIdx.x >> 4);
    const bool live = ix < a.nx && iy < a.ny;
    const double gx0 = a.xax[live ? ix : 0], gy0 = a.yax[live ? iy : 0];
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
    if (live) a.part[((size_t)blockIdx.z * a.chunks + blockIdx.y) * n_pix + (size_t)iy * a.nx + ix] = make_double2(acc_re, acc_im);
}

// tdbp_tile_kernel with the prologue lane forming w of this hypothesis
__global__ __launch_bounds__(256) void tdbp_search_tile_kernel(SearchArgs a) {
    __shared__ TilePulse s_tp[TP_BATCH];
    const int tiles_x = (a.nx + 15) >> 4;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int ix = tx * 16 + (threadIdx.x & 15), iy = ty * 16 + (threadIdx.x >> 4);
    const bool live = ix < a.nx && iy < a.ny;
    const double xc = a.xax[min(tx * 16 + 8, a.nx - 1)], yc = a.yax[min(ty * 16 + 8, a.ny - 1)];
    const double qx = a.xax[live ? ix : 0] - xc, qy = a.yax[live ? iy : 0] - yc;
    const double q2 = fma(qx, qx, qy * qy);
    const float qxf = (float)qx, qyf = (float)qy;
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
            const double dx = fma(vfx, g.dt, xc) - g.px, dy = fma(vfy, g.dt, yc) - g.py, dz = vfz * g.dt - g.pz;
            s_tp[threadIdx.x] = tdbp_tile_prologue(a, dx, dy, dz, wx, wy, wz, w2);
        }
        __syncthreads();
        for (int k = 0; k < nb; ++k) tdbp_tile_pixel(a, s_tp[k], qx, qy, q2, qxf, qyf, two_inv_ns, pb + k, acc_re, acc_im);
    }
    const size_t n_pix = (size_t)a.nx * a.ny;
    if (live) a.part[((size_t)blockIdx.z * a.chunks + blockIdx.y) * n_pix + (size_t)iy * a.nx + ix] = make_double2(acc_re, acc_im);
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

struct TdbpSearch {
    SearchGeo *geo = nullptr, *h_geo = nullptr;            // device table and its page-locked staging
    double *hyps = nullptr, *h_hyps = nullptr;             // [MAX_HYP][3]
    hipEvent_t up_done = nullptr;                          // the uploads of the last call have read the staging
    double2* part = nullptr;
    size_t part_cap = 0;                                   // double2 elements
    sarx_tdbp_search_record* rec = nullptr;                // staging of the host entry point
    double2* stack = nullptr;
    size_t stack_cap = 0;
    int route = -1;
};

void tdbp_search_free(TdbpSearch* s) {
    if (!s) return;
    hipFree(s->geo); hipFree(s->hyps); hipFree(s->part); hipFree(s->rec); hipFree(s->stack);
    if (s->h_geo) hipHostFree(s->h_geo);
    if (s->h_hyps) hipHostFree(s->h_hyps);
    if (s->up_done) hipEventDestroy(s->up_done);
    delete s;
}

#define SCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

static hipError_t search_scratch(Tdbp* t, TdbpSearch** out) {
    if (!t->search) {
        TdbpSearch* s = new TdbpSearch();
        hipError_t e = hipMalloc(&s->geo, (size_t)t->n_p * sizeof(SearchGeo));
        if (e == hipSuccess) e = hipHostMalloc(&s->h_geo, (size_t)t->n_p * sizeof(SearchGeo), hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(&s->hyps, (size_t)SARX_TDBP_SEARCH_MAX_HYP * 3 * sizeof(double));
        if (e == hipSuccess) e = hipHostMalloc(&s->h_hyps, (size_t)SARX_TDBP_SEARCH_MAX_HYP * 3 * sizeof(double), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->up_done, hipEventDisableTiming);
        if (e != hipSuccess) { tdbp_search_free(s); return e; }
        t->search = s;
    }
    *out = t->search;
    return hipSuccess;
}

static hipError_t grow(double2** buf, size_t* cap, size_t need) {
    if (need <= *cap) return hipSuccess;
    SCK(hipFree(*buf));                                    // waits for the launches that may still read it
    *buf = nullptr; *cap = 0;
    SCK(hipMalloc(buf, need * sizeof(double2)));
    *cap = need;
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
    SCK(search_scratch(t, &s));
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
    SCK(tdbp_range_compress(t, raw, lo, hi, st));
    SCK(hipEventSynchronize(s->up_done));                  // the previous call's uploads have left the staging (at once as a rule)
    for (int p = 0; p < n_p; ++p) {
        SearchGeo& g = s->h_geo[p];
        g.px = geo[p].px; g.py = geo[p].py; g.pz = geo[p].pz;
        g.vx = vel[3 * p]; g.vy = vel[3 * p + 1]; g.vz = vel[3 * p + 2];
        g.dt = geo[p].dt; g.pad = 0.0;
    }
    memcpy(s->h_hyps, vel_hyps, (size_t)n_hyp * 3 * sizeof(double));
    SCK(hipMemcpyAsync(s->geo, s->h_geo, (size_t)n_p * sizeof(SearchGeo), hipMemcpyHostToDevice, st));
    SCK(hipMemcpyAsync(s->hyps, s->h_hyps, (size_t)n_hyp * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    SCK(hipEventRecord(s->up_done, st));
    SCK(tdbp_ensure_axes(t, scene_size, st));
    // pulse chunks: enough workgroups to fill the device several times over, never fewer than 32 pulses each; fewer chunks with
    // more hypotheses, so the partial images stay near 16384 workgroups x 4 KiB
    const int tiles = ((t->nx + 15) / 16) * ((t->ny + 15) / 16);
    if (chunks < 1) {
        const long long blocks = (long long)tiles * n_hyp;
        chunks = (int)((16384 + blocks - 1) / blocks);
        if (chunks > n_p / 32) chunks = n_p / 32;
    }
    if (chunks > SARX_TDBP_SEARCH_MAX_CHUNKS) chunks = SARX_TDBP_SEARCH_MAX_CHUNKS;
    if (chunks > n_p) chunks = n_p;
    if (chunks < 1) chunks = 1;
    const int per_chunk = (n_p + chunks - 1) / chunks;
    chunks = (n_p + per_chunk - 1) / per_chunk;
    SCK(grow(&s->part, &s->part_cap, (size_t)n_hyp * chunks * t->nx * t->ny));
    SearchArgs a{};
    tdbp_fill_args(t, t_start, per_chunk, a);
    a.geo = s->geo; a.hyps = s->hyps; a.part = s->part; a.chunks = chunks;
    const dim3 grid(tiles, chunks, n_hyp);
    if (tile) hipLaunchKernelGGL(tdbp_search_tile_kernel, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tdbp_search_kernel, grid, dim3(256), 0, st, a);
    SCK(hipGetLastError());
    s->route = tile ? 1 : 0;
    return launch_metric(t, s->part, chunks, n_hyp, d_images, d_records, st);
}

hipError_t tdbp_search_metric(Tdbp* t, const double2* d_stack, int n_hyp, sarx_tdbp_search_record* d_records, hipStream_t st) {
    return launch_metric(t, d_stack, 1, n_hyp, nullptr, d_records, st);
}

int tdbp_search_route(const Tdbp* t) { return t->search ? t->search->route : -1; }

hipError_t tdbp_search_staging(Tdbp* t, int n_hyp, bool images, sarx_tdbp_search_record** d_records, double2** d_images, hipStream_t st) {
    TdbpSearch* s = nullptr;
    SCK(search_scratch(t, &s));
    if (!s->rec) SCK(hipMalloc(&s->rec, (size_t)SARX_TDBP_SEARCH_MAX_HYP * sizeof(sarx_tdbp_search_record)));
    *d_records = s->rec;
    *d_images = nullptr;
    if (images) {
        SCK(grow(&s->stack, &s->stack_cap, (size_t)n_hyp * t->nx * t->ny));
        *d_images = s->stack;
    }
    return hipSuccess;
}

}  // namespace sarx
