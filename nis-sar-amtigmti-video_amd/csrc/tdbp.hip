// Time-domain back-projection for the VideoSAR batch: tdbp_gpu, sar_batch_sim.py:171-238.
//
//   1 range compression (:180-185): circular correlation of every pulse [num_samples] with the fftshifted
//     reference chirp (int(T_P*FS) taps).  num_samples is 22004 = 4 * 5501 natively, so the correlation
//     runs as overlap-save blocks on the power-of-two line FFT (M <= 32768): block b produces outputs
//     [b*B, b*B + B), B = M - taps + 1, from the wrapped input segment starting at b*B.
//   2 back-projection (:197-236): for every pixel and pulse the two-way delay with the receiver moved by
//     the platform during the flight time (:216-220), the range-Doppler coupling shift (:209-213), a linear
//     interpolation of the compressed pulse and the carrier phase exp(j 2 pi FC tau) (:231), summed over
//     pulses.  Geometry and phase argument in fp64 (FC*tau = 3e7 revolutions); the interpolation
//     coordinate goes through float32 exactly as the reference's F.grid_sample call does (:223-226:
//     normalise, cast, unnormalise with one fused multiply-add), because that quantisation (1e-3 sample)
//     is visible at the 1e-4 parity bar; samples fp32, pulse sum fp64.
//     One thread per pixel (16 x 16 pixel tiles keep a wave's gather inside a few hundred bytes of one
//     pulse), pulses split into chunks across blockIdx.y, partial images reduced in a fixed order.  The arithmetic of
//     one pixel and pulse is tdbp_pixel.hpp's, which the focus-velocity search (tdbp_search.hip) runs too.
//     Compute-bound in fp64 (one rsqrt + a short series instead of two square roots and a division):
//     6.6e8 pixel-pulses per 512 x 512 x 2500 frame in 1.66 ms.
//   3 what the search and the two-receiver pair (tdbp_pair.hip) share with the focus on the host, stated here once (tdbp_plan.h):
//     tdbp_range_compress into a destination the caller names, the geometry bounds (moved_rect_range, tdbp_clamp_window,
//     tdbp_tile_reach), the pulse chunks of one call (tdbp_pick_chunks) and the scratch either holds beside the plan (TdbpScratch, TdbpHypScratch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>

#include "general.h"
#include "tdbp_plan.h"

namespace sarx {

typedef std::complex<double> zd;

struct TdbpArgs {
    const cf* rc;            // [n_p][n_s] range-compressed pulses
    const PulseGeo* geo;
    const double *xax, *yax;
    double2* part;           // [chunks][ny*nx]
    double vfx, vfy, vfz;
    double inv_c, fc, fs, t_start, k_shift, inv_ns;
    float half_w;
    int n_p, n_s, nx, ny, per_chunk;
};

__global__ __launch_bounds__(256) void wrap_copy_kernel(const cf* in, int rows, int n, cf* out, int m, int col0) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int s = (col0 + j) % n;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) out[(size_t)r * m + j] = in[(size_t)r * n + s];
}

__global__ __launch_bounds__(256) void tdbp_kernel(TdbpArgs a) {
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const double gx0 = a.xax[px.live ? px.ix : 0], gy0 = a.yax[px.live ? px.iy : 0];
    const int p0 = blockIdx.y * a.per_chunk, p1 = min(a.n_p, p0 + a.per_chunk);
    double acc_re = 0.0, acc_im = 0.0;
    for (int p = p0; p < p1; ++p) {
        const PulseGeo g = a.geo[p];
        // pixel moved with the focus velocity (:205), vector to the transmitter (:207-208)
        const double dx = fma(a.vfx, g.dt, gx0) - g.px;
        const double dy = fma(a.vfy, g.dt, gy0) - g.py;
        const double dz = a.vfz * g.dt - g.pz;
        tdbp_exact_pixel(a, dx, dy, dz, g.wx, g.wy, g.wz, g.pad, p, acc_re, acc_im);
    }
    if (px.live) a.part[(size_t)blockIdx.y * a.nx * a.ny + (size_t)px.iy * a.nx + px.ix] = make_double2(acc_re, acc_im);
}

// the tile form (tdbp_pixel.hpp): one lane per pulse fills the batch's records, then every pixel walks them
__global__ __launch_bounds__(256) void tdbp_tile_kernel(TdbpArgs a) {
    __shared__ TilePulse s_tp[TP_BATCH];
    const TdbpPix px = tdbp_pix(a.nx, a.ny);
    const TdbpTileOffsets o = tdbp_tile_offsets(a.xax, a.yax, px, a.nx, a.ny);
    const float qxf = (float)o.qx, qyf = (float)o.qy;
    const int p0 = blockIdx.y * a.per_chunk, p1 = min(a.n_p, p0 + a.per_chunk);
    const double two_inv_ns = 2.0 * a.inv_ns;
    double acc_re = 0.0, acc_im = 0.0;
    for (int pb = p0; pb < p1; pb += TP_BATCH) {
        const int nb = min(TP_BATCH, p1 - pb);
        __syncthreads();                                   // the previous batch has been consumed
        if ((int)threadIdx.x < nb) {
            const PulseGeo g = a.geo[pb + threadIdx.x];
            const double dx = fma(a.vfx, g.dt, o.xc) - g.px, dy = fma(a.vfy, g.dt, o.yc) - g.py, dz = a.vfz * g.dt - g.pz;   // :205-208 at the reference pixel
            s_tp[threadIdx.x] = tdbp_tile_prologue(a, dx, dy, dz, g.wx, g.wy, g.wz, g.pad);
        }
        __syncthreads();
        for (int k = 0; k < nb; ++k) tdbp_tile_pixel(a, s_tp[k], o.qx, o.qy, o.q2, qxf, qyf, two_inv_ns, pb + k, acc_re, acc_im);
    }
    if (px.live) a.part[(size_t)blockIdx.y * a.nx * a.ny + (size_t)px.iy * a.nx + px.ix] = make_double2(acc_re, acc_im);
}

__global__ __launch_bounds__(256) void tdbp_reduce_kernel(const double2* part, int chunks, size_t n_pix, double2* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pix) return;
    out[i] = tdbp_sum_chunks(part, chunks, n_pix, i);
}

void tdbp_destroy(Tdbp* t) {
    if (!t) return;
    for (auto& kv : t->hhat) hipFree(kv.second);
    hipFree(t->work); hipFree(t->rc); hipFree(t->xax); hipFree(t->yax);
    for (int b = 0; b < 2; ++b) {
        hipFree(t->geo[b]);
        if (t->h_geo[b]) hipHostFree(t->h_geo[b]);
        if (t->geo_done[b]) hipEventDestroy(t->geo_done[b]);
    }
    hipFree(t->part); hipFree(t->img);
    tdbp_search_free(t->search);
    tdbp_rx_free(t->pair);
    tdbp_pair_search_free(t->pair_search);
    tdbp_rx_free(t->multi);
    delete t;
}

// conj(FFT_m(fftshift(ref_chirp))) (:177-179) for an m-point transform, cached; linspace endpoints as torch builds
// them (two-sided)
static hipError_t filter_spectrum(Tdbp* t, int m, cf** out) {
    auto it = t->hhat.find(m);
    if (it != t->hhat.end()) { if (out) *out = it->second; return hipSuccess; }
    const int l_ref = t->l_ref;
    const sarx_tdbp_params* k = &t->k;
    std::vector<zd> h(m, zd(0, 0));
    const double step = l_ref > 1 ? k->t_p / (double)(l_ref - 1) : 0.0;
    for (int i = 0; i < t->taps; ++i) {
        const int src = ((i - l_ref / 2) % l_ref + l_ref) % l_ref;     // fftshift: out[i] = ref[(i - L//2) mod L]
        const double tt = src < l_ref / 2 ? -k->t_p / 2 + step * (double)src : k->t_p / 2 - step * (double)(l_ref - 1 - src);
        h[i] = std::polar(1.0, M_PI * k->k_rate * tt * tt);
    }
    host_fft_pow2(h);
    for (auto& v : h) v = std::conj(v);
    if (m == 32768) to_split_order(h);
    std::vector<cf> hf(m);
    for (int i = 0; i < m; ++i) hf[i] = make_float2((float)h[i].real(), (float)h[i].imag());
    cf* d = nullptr;
    TCK(hipMalloc(&d, (size_t)m * sizeof(cf)));
    hipError_t e = hipMemcpy(d, hf.data(), (size_t)m * sizeof(cf), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(d); return e; }
    t->hhat[m] = d;
    if (out) *out = d;
    return hipSuccess;
}

Tdbp* tdbp_create(int n_pulses, int num_samples, int nx, int ny, const sarx_tdbp_params* k, const float2* tw_all,
                  std::string& err) {
    const int l_ref = (int)(k->t_p * k->fs);                           // int(T_P * FS), :177
    if (l_ref < 1) { err = "T_P * FS must be >= 1 sample"; return nullptr; }
    const int taps = l_ref < num_samples ? l_ref : num_samples;       // fft(..., n=num_samples) truncates
    int m = 16;
    while (m < num_samples + taps - 1 && m < 32768) m <<= 1;
    if (m - taps + 1 < m / 2) { err = "reference chirp longer than 16385 samples"; return nullptr; }
    Tdbp* t = new Tdbp();
    t->n_p = n_pulses; t->n_s = num_samples; t->nx = nx; t->ny = ny; t->taps = taps; t->m = m; t->blk = m - taps + 1;
    t->k = *k; t->tw_all = tw_all;
    const size_t n_pix = (size_t)nx * ny;
    // a policy of its own, not tdbp_pick_chunks: fixed when the plan is made, and capped by the bytes of the partial images
    int chunks = (int)(((size_t)1 << 20) / (n_pix ? n_pix : 1));
    if (chunks > n_pulses / 32) chunks = n_pulses / 32;
    if (chunks > 64) chunks = 64;
    if (chunks < 1) chunks = 1;
    t->per_chunk = (n_pulses + chunks - 1) / chunks;
    t->chunks = (n_pulses + t->per_chunk - 1) / t->per_chunk;
    auto bail = [&](const char* what, hipError_t e) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        tdbp_destroy(t);
        return (Tdbp*)nullptr;
    };
    hipError_t e;
    t->l_ref = l_ref;
    if (const char* ev = getenv("SARX_TDBP_FULL_RC")) t->full_rc = atoi(ev) != 0;
    if (const char* ev = getenv("SARX_TDBP_RC_FUSED")) t->three_launch = atoi(ev) == 0;
    if ((e = filter_spectrum(t, m, nullptr)) != hipSuccess) return bail("filter spectrum", e);
    if ((e = hipMalloc(&t->work, (size_t)n_pulses * m * sizeof(cf))) != hipSuccess) return bail("hipMalloc work", e);
    if ((e = hipMalloc(&t->rc, (size_t)n_pulses * num_samples * sizeof(cf))) != hipSuccess) return bail("hipMalloc", e);
    for (int b = 0; b < 2; ++b) {
        if ((e = hipMalloc(&t->geo[b], (size_t)n_pulses * sizeof(PulseGeo))) != hipSuccess) return bail("hipMalloc", e);
        if ((e = hipHostMalloc(&t->h_geo[b], (size_t)n_pulses * sizeof(PulseGeo), hipHostMallocDefault)) != hipSuccess) return bail("hipHostMalloc", e);
        if ((e = hipEventCreateWithFlags(&t->geo_done[b], hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    }
    if ((e = hipMalloc(&t->xax, (size_t)nx * sizeof(double))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&t->yax, (size_t)ny * sizeof(double))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&t->part, (size_t)t->chunks * n_pix * sizeof(double2))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&t->img, n_pix * sizeof(double2))) != hipSuccess) return bail("hipMalloc", e);
    t->bytes = (uint64_t)n_pulses * (m + num_samples) * sizeof(cf) + (uint64_t)(t->chunks + 1) * n_pix * sizeof(double2);
    return t;
}

// outputs [n0, n0 + cnt) of the circular correlation through one m-point transform (cnt <= m - taps + 1)
static hipError_t compress_block(Tdbp* t, const float2* raw, cf* dst, int n0, int cnt, int m, hipStream_t st) {
    cf* hhat = nullptr;
    TCK(filter_spectrum(t, m, &hhat));
    const int n = t->n_s;
    if (m <= 16384 && !t->three_launch) {
        // one launch: the wrapped m-sample segment read straight from the pulse, FFT . conj(reference spectrum) . IFFT in
        // registers / LDS, the cnt wanted outputs written to their place (range_pass_kernel<m, RG_CONV>): 0.42 -> 0.185 ms per
        // 2500 x 22004 frame against copy-in, two transforms and copy-out (profiles/r05_bj_*)
        RangeArgs ca{};
        ca.in = raw; ca.out = dst + n0; ca.tw = t->tw_all + m; ca.n_az = t->n_p; ca.inv_n = 1.0f / (float)m;
        ca.mulvec = hhat; ca.mul_period = 1;
        ca.conv_valid = m; ca.conv_crop0 = 0; ca.conv_out = cnt; ca.conv_in_ld = (size_t)n; ca.conv_out_ld = (size_t)n;
        ca.conv_wrap_n = n; ca.conv_wrap_c0 = n0 % n;
        return launch_range_pass(m, RG_CONV, ca, st);
    }
    dim3 grid((m + 255) / 256, t->n_p < 8192 ? t->n_p : 8192);
    hipLaunchKernelGGL(wrap_copy_kernel, grid, dim3(256), 0, st, raw, t->n_p, n, t->work, m, n0);
    TCK(hipGetLastError());
    TCK(line_fft_pow2(t->tw_all, t->work, t->n_p, m, false, st, hhat));      // * conj(reference spectrum) in the epilogue
    TCK(line_fft_pow2(t->tw_all, t->work, t->n_p, m, true, st));
    return scale_copy_cols(t->work, t->n_p, cnt, m, dst + n0, t->n_p, cnt, n, nullptr, 1.0f, st);
}

// raw: device [n_p][n_s] complex64.  Leaves the range-compressed samples [lo, hi) of every pulse in dst [n_p][n_s]: the plan's rc, or
// the pair's buffer for its second channel (the back-projection of one scene reads a narrow window of each pulse: ~1700 of 22004
// samples natively).
hipError_t tdbp_range_compress(Tdbp* t, const float2* raw, cf* dst, int lo, int hi, hipStream_t st) {
    const int n = t->n_s;
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    t->win_lo = lo; t->win_hi = hi;
    if (hi <= lo) return hipSuccess;
    int m = 16;
    while (m < (hi - lo) + t->taps - 1) m <<= 1;
    if (m < t->m) return compress_block(t, raw, dst, lo, hi - lo, m, st);        // one transform shorter than the plan's
    for (int n0 = lo; n0 < hi; n0 += t->blk) {
        const int cnt = (hi - n0 < t->blk) ? hi - n0 : t->blk;
        TCK(compress_block(t, raw, dst, n0, cnt, t->m, st));
    }
    return hipSuccess;
}

// ---- geometry bounds on the host: what the focus, the search and the pair decide their sample window and their kernel with ----
// Nearest and farthest transmit range of one pulse over the pixel rectangle (half side h) moved by v_f dt: the rectangle is
// convex, so the range is largest at a corner and smallest at the projection of the platform clamped to the rectangle.
void moved_rect_range(const PulseGeo& g, const double* vf, double h, double* dmin, double* dmax) {
    const double sx = vf[0] * g.dt, sy = vf[1] * g.dt, gz = vf[2] * g.dt - g.pz;
    const double qx = g.px - sx, qy = g.py - sy;                        // platform relative to the moved rectangle
    const double cx = qx < -h ? -h : (qx > h ? h : qx), cy = qy < -h ? -h : (qy > h ? h : qy);
    *dmin = sqrt((cx - qx) * (cx - qx) + (cy - qy) * (cy - qy) + gz * gz);
    const double ax = fabs(qx) + h, ay = fabs(qy) + h;                  // farthest corner
    *dmax = sqrt(ax * ax + ay * ay + gz * gz);
}

// Sample indices [imin, imax] (fractional) to the window [lo, hi) inside [0, n_s]: x = idx - 0.5 rounded through float32 (< 1 sample
// at any n_s <= 2^23), i0 = floor(x), i0 + 1 is read too.  A NaN bound gives 0, never a cast of it.
void tdbp_clamp_window(double imin, double imax, int n_s, int* lo, int* hi) {
    const double l = floor(imin) - 3.0, u = ceil(imax) + 4.0;
    *lo = !(l > 0) ? 0 : (l > (double)n_s ? n_s : (int)l);
    *hi = !(u > 0) ? 0 : (u > (double)n_s ? n_s : (int)u);
}

// Farthest pixel of a 16 x 16 tile from its reference pixel (index 8 of 16), in metres; negative when the grid is thinner than two pixels
double tdbp_tile_reach(const Tdbp* t, double scene_size) {
    if (t->nx < 2 || t->ny < 2) return -1.0;
    return 8.0 * hypot(scene_size / (double)(t->nx - 1), scene_size / (double)(t->ny - 1));
}

// Sample window [lo, hi) that the back-projection can touch: a bound, not an estimate.  Per pulse the transmit range lies in
// moved_rect_range; |d_rx - d_tx| <= |v_rel| tau_a and |t_shift| <= |v_rel| |k_shift| (:209-219).
void tdbp_sample_window(const Tdbp* t, const std::vector<PulseGeo>& geo, const double* vf, double t_start, double scene_size,
                        int* lo, int* hi) {
    const double c = t->k.c, fs = t->k.fs, ks = fabs(t->k.fc * 2.0 / t->k.c / t->k.k_rate), h = scene_size / 2;
    double imin = 1e300, imax = -1e300;
    for (const PulseGeo& g : geo) {
        double dmin, dmax;
        moved_rect_range(g, vf, h, &dmin, &dmax);
        const double w = sqrt(g.wx * g.wx + g.wy * g.wy + g.wz * g.wz);
        const double slack = w * (2.0 * dmax / c);
        const double a = ((2.0 * dmin - slack) / c - t_start - w * ks) * fs;
        const double b = ((2.0 * dmax + slack) / c - t_start + w * ks) * fs;
        if (a < imin) imin = a;
        if (b > imax) imax = b;
    }
    tdbp_clamp_window(imin, imax, t->n_s, lo, hi);
}

// May the tile kernel stand in for the exact one?  The tile's reach (tdbp_tile_reach) against the nearest range of any pulse: the
// first omitted series term of d_tx, 5 u^4 / 128 * d, must stay below 1e-9 m (4e-7 rad of carrier phase at X band).
// SARX_TDBP_TILE=0 forces the exact kernel (A/B).
bool tdbp_tile_ok(const Tdbp* t, const std::vector<PulseGeo>& geo, const double* vf, double scene_size) {
    if (const char* ev = getenv("SARX_TDBP_TILE")) if (atoi(ev) == 0) return false;
    const double h = scene_size / 2, qm = tdbp_tile_reach(t, scene_size);
    if (qm < 0.0) return false;
    for (const PulseGeo& g : geo) {
        double dmin, dmax;
        moved_rect_range(g, vf, h, &dmin, &dmax);
        if (!(dmin > 0.0)) return false;
        const double u = 2.0 * qm / dmin + (qm / dmin) * (qm / dmin);
        if (!(5.0 / 128.0 * u * u * u * u * dmax < 1e-9)) return false;
    }
    return true;
}

// ---- what a call of the search or the pair chooses and holds beside the plan ----
// Pulse chunks of one call: requested > 0 is the caller's number (sarx_tdbp_search_set_chunks); else enough workgroups to fill the
// device several times over - 16384 of them, a chunk launching tiles x blocks_per_chunk - and never fewer than 32 pulses each.
// Returns the chunks that hold a pulse, *per_chunk pulses in each but the last.
int tdbp_pick_chunks(int tiles, int blocks_per_chunk, int n_pulses, int requested, int* per_chunk) {
    int chunks = requested;
    if (chunks < 1) {
        const long long blocks = (long long)tiles * blocks_per_chunk;
        chunks = (int)((16384 + blocks - 1) / blocks);
        if (chunks > n_pulses / 32) chunks = n_pulses / 32;
    }
    if (chunks > SARX_TDBP_SEARCH_MAX_CHUNKS) chunks = SARX_TDBP_SEARCH_MAX_CHUNKS;
    if (chunks > n_pulses) chunks = n_pulses;
    if (chunks < 1) chunks = 1;
    *per_chunk = (n_pulses + chunks - 1) / chunks;
    return (n_pulses + *per_chunk - 1) / *per_chunk;
}

hipError_t grow(double2** buf, size_t* cap, size_t need) {
    if (need <= *cap) return hipSuccess;
    TCK(hipFree(*buf));                                    // waits for the launches that may still read it
    *buf = nullptr; *cap = 0;
    TCK(hipMalloc(buf, need * sizeof(double2)));
    *cap = need;
    return hipSuccess;
}

hipError_t tdbp_scratch_init(TdbpScratch* s, int n_p, size_t bytes) {
    s->bytes = (size_t)n_p * bytes;
    TCK(hipMalloc(&s->geo, s->bytes));
    TCK(hipHostMalloc(&s->h_geo, s->bytes, hipHostMallocDefault));
    return hipEventCreateWithFlags(&s->up_done, hipEventDisableTiming);
}

void tdbp_scratch_free(TdbpScratch* s) {
    hipFree(s->geo); hipFree(s->part);
    if (s->h_geo) hipHostFree(s->h_geo);
    if (s->up_done) hipEventDestroy(s->up_done);
}

hipError_t tdbp_hyp_scratch_init(TdbpHypScratch* s, int n_p, size_t bytes, int max_hyp) {
    TCK(tdbp_scratch_init(s, n_p, bytes));
    TCK(hipMalloc(&s->hyps, (size_t)max_hyp * 3 * sizeof(double)));
    return hipHostMalloc(&s->h_hyps, (size_t)max_hyp * 3 * sizeof(double), hipHostMallocDefault);
}

void tdbp_hyp_scratch_free(TdbpHypScratch* s) {
    tdbp_scratch_free(s);
    hipFree(s->hyps);
    if (s->h_hyps) hipHostFree(s->h_hyps);
}

static void linspace(double a, double b, int n, std::vector<double>& out) {     // numpy.linspace (:173-174)
    out.resize(n);
    const double step = n > 1 ? (b - a) / (double)(n - 1) : 0.0;
    for (int i = 0; i < n; ++i) out[i] = (double)i * step + a;
    if (n > 1) out[n - 1] = b;
}

hipError_t tdbp_ensure_axes(Tdbp* t, double scene_size, hipStream_t st) {     // pixel axes: once per scene size (a frame loop keeps it)
    if (t->axes_scene == scene_size) return hipSuccess;
    std::vector<double> xa, ya;
    linspace(-scene_size / 2, scene_size / 2, t->nx, xa);
    linspace(-scene_size / 2, scene_size / 2, t->ny, ya);
    TCK(hipStreamSynchronize(st));                         // an earlier focus may still read the old axes
    TCK(hipMemcpy(t->xax, xa.data(), xa.size() * sizeof(double), hipMemcpyHostToDevice));
    TCK(hipMemcpy(t->yax, ya.data(), ya.size() * sizeof(double), hipMemcpyHostToDevice));
    t->axes_scene = scene_size;
    return hipSuccess;
}

void tdbp_pulse_table(const Tdbp* t, const double* pos, const double* t_pulses, std::vector<PulseGeo>& geo) {
    geo.assign(t->n_p, PulseGeo{});
    double mean = 0.0;
    for (int p = 0; p < t->n_p; ++p) mean += t_pulses[p];
    mean /= (double)t->n_p;
    for (int p = 0; p < t->n_p; ++p) {
        PulseGeo& g = geo[p];
        g.px = pos[3 * p]; g.py = pos[3 * p + 1]; g.pz = pos[3 * p + 2];
        g.dt = t_pulses[p] - mean;
    }
}

void tdbp_set_focus(std::vector<PulseGeo>& geo, const double* vel, const double* vf) {
    for (size_t p = 0; p < geo.size(); ++p) {
        PulseGeo& g = geo[p];
        g.wx = vel[3 * p] - vf[0]; g.wy = vel[3 * p + 1] - vf[1]; g.wz = vel[3 * p + 2] - vf[2];
        g.pad = g.wx * g.wx + g.wy * g.wy + g.wz * g.wz;
    }
}

// raw: device [n_p][n_s]; pos, vel: host [n_p][3]; t_pulses: host [n_p].  Result in t->img (device, complex128 [ny][nx]).
// all_samples: compress every sample of every pulse (the caller wants rc_data), else only the window the scene can touch
hipError_t tdbp_focus(Tdbp* t, const float2* raw, const double* pos, const double* vel, const double* t_pulses, double t_start,
                      const double* vel_focus, double scene_size, bool all_samples, hipStream_t st) {
    const int slot = (t->geo_slot ^= 1);
    TCK(hipEventSynchronize(t->geo_done[slot]));           // the focus two calls ago has finished with this slot (returns at once as a rule)
    std::vector<PulseGeo> geo;
    tdbp_pulse_table(t, pos, t_pulses, geo);
    tdbp_set_focus(geo, vel, vel_focus);
    int lo = 0, hi = t->n_s;
    if (!all_samples && !t->full_rc) tdbp_sample_window(t, geo, vel_focus, t_start, scene_size, &lo, &hi);
    TCK(tdbp_range_compress(t, raw, t->rc, lo, hi, st));
    memcpy(t->h_geo[slot], geo.data(), geo.size() * sizeof(PulseGeo));
    TCK(hipMemcpyAsync(t->geo[slot], t->h_geo[slot], geo.size() * sizeof(PulseGeo), hipMemcpyHostToDevice, st));
    TCK(tdbp_ensure_axes(t, scene_size, st));
    TdbpArgs a{};
    tdbp_fill_args(t, t_start, t->per_chunk, a);
    a.geo = t->geo[slot]; a.part = t->part;
    a.vfx = vel_focus[0]; a.vfy = vel_focus[1]; a.vfz = vel_focus[2];
    const int tiles = ((t->nx + 15) / 16) * ((t->ny + 15) / 16);
    if (tdbp_tile_ok(t, geo, vel_focus, scene_size)) hipLaunchKernelGGL(tdbp_tile_kernel, dim3(tiles, t->chunks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tdbp_kernel, dim3(tiles, t->chunks), dim3(256), 0, st, a);
    TCK(hipGetLastError());
    const size_t n_pix = (size_t)t->nx * t->ny;
    hipLaunchKernelGGL(tdbp_reduce_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st, t->part, t->chunks, n_pix, t->img);
    TCK(hipGetLastError());
    return hipEventRecord(t->geo_done[slot], st);
}

const double2* tdbp_image(const Tdbp* t) { return t->img; }
const float2* tdbp_rc(const Tdbp* t) { return t->rc; }
void tdbp_window(const Tdbp* t, int* lo, int* hi) { *lo = t->win_lo; *hi = t->win_hi; }
uint64_t tdbp_bytes(const Tdbp* t) { return t->bytes; }

}  // namespace sarx
