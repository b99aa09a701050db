// One pixel and pulse of the time-domain back-projection (sar_batch_sim.py:205-232), stated once for the focus kernels of tdbp.hip,
// the focus-velocity search kernels of tdbp_search.hip, the N-receiver kernels of tdbp_multi.hip and the two-receiver search per GMTI
// report (tdbp_pair_search.hip), with what stands around it in every one of them: the tile and pixel coordinates of a thread (tdbp_pix), a
// pixel's offset from its tile's reference pixel (tdbp_tile_offsets) and the fixed-order sum of a pixel's chunks (tdbp_sum_chunks).
// A single-channel kernel keeps only where the focus velocity v_f and w = v_plat - v_f come from, the batch loop of the tile form and the
// place of its partial image; the whole pulse loops of N = 2, 3 or 4 receivers are here (tdbp_multi_pulses, tdbp_multi_tile_pulses), for
// the kernels of tdbp_multi.hip and, at N = 2, for the pair and the kernels of its search.
// Every statement groups its operands as the reference parity (1e-4) was measured with: -ffp-contract=on fuses inside a statement
// only, so splitting or merging one changes bits.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_core.hpp"

namespace sarx {

// One thread per pixel, 256 threads on a 16 x 16 pixel tile, tiles row by row along blockIdx.x.  A dead lane (ragged right and
// bottom tiles) runs the whole pulse loop on pixel 0's coordinates - the barriers of the tile form need it - and stores nothing.
struct TdbpPix { int tx, ty, ix, iy; bool live; };
__device__ __forceinline__ TdbpPix tdbp_pix(int nx, int ny) {
    const int tiles_x = (nx + 15) >> 4;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int ix = tx * 16 + (threadIdx.x & 15), iy = ty * 16 + (threadIdx.x >> 4);
    return {tx, ty, ix, iy, ix < nx && iy < ny};
}

// the tile's reference pixel (index 8 of 16, clamped to the grid) and this pixel's offset q from it: exact differences of the axis tables
struct TdbpTileOffsets { double xc, yc, qx, qy, q2; };
__device__ __forceinline__ TdbpTileOffsets tdbp_tile_offsets(const double* xax, const double* yax, const TdbpPix& px, int nx, int ny) {
    const double xc = xax[min(px.tx * 16 + 8, nx - 1)], yc = yax[min(px.ty * 16 + 8, ny - 1)];
    const double qx = xax[px.live ? px.ix : 0] - xc, qy = yax[px.live ? px.iy : 0] - yc;
    return {xc, yc, qx, qy, fma(qx, qx, qy * qy)};
}

// src: [chunks][n_pix] partial images; the sum of pixel i over the chunks, c rising: the same bits on every run
__device__ __forceinline__ double2 tdbp_sum_chunks(const double2* src, int chunks, size_t n_pix, size_t i) {
    double re = 0.0, im = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double2 v = src[(size_t)c * n_pix + i];
        re += v.x;
        im += v.y;
    }
    return make_double2(re, im);
}

// A: the kernel's argument struct (TdbpArgs, SearchArgs); read here: rc [n_p][n_s], n_s, half_w, inv_c, fc, fs, t_start, k_shift,
// inv_ns - the fields tdbp_fill_args (tdbp_plan.h) sets.

// the compressed pulse p at the normalised coordinate xn, as F.grid_sample reads it, times the carrier phase; summed in fp64
template <class A> __device__ __forceinline__ void tdbp_sample(const A& c, float xn, double tau, int p, double& acc_re, double& acc_im) {
    const float x = __fmaf_rn(xn + 1.0f, c.half_w, -0.5f);                                  // grid_sample unnormalise
    const float x0 = floorf(x);
    const float w = x - x0, e = 1.0f - w;
    const int i0 = (int)x0;
    const cf* row = c.rc + (size_t)p * c.n_s;
    cf v0 = make_float2(0.f, 0.f), v1 = v0;
    if (i0 >= 0 && i0 < c.n_s) v0 = row[i0];
    if (i0 + 1 >= 0 && i0 + 1 < c.n_s) v1 = row[i0 + 1];
    const float s_re = fmaf(v1.x, w, v0.x * e), s_im = fmaf(v1.y, w, v0.y * e);
    const cf ph = cis_rev(c.fc * tau);                                                      // :231-232
    acc_re += (double)(s_re * ph.x - s_im * ph.y);
    acc_im += (double)(s_re * ph.y + s_im * ph.x);
}

// The exact form.  d: from the transmitter to the pixel moved with the focus velocity (:205-208); w = v_rel (:211), w2 = |w|^2.
template <class A> __device__ __forceinline__ void tdbp_exact_pixel(const A& c, double dx, double dy, double dz, double wx, double wy,
                                                                   double wz, double w2, int p, double& acc_re, double& acc_im) {
    const double s_tx = fma(dx, dx, fma(dy, dy, dz * dz));
    const double inv_d = rsqrt(s_tx);                                                       // one reciprocal square root
    const double d_tx = s_tx * inv_d;                                                       // serves range and unit vector
    const double dw = wx * dx + wy * dy + wz * dz;
    const double v_rad = dw * inv_d;                                                        // :210-212
    const double t_shift = v_rad * c.k_shift;                                               // :213
    const double tau_a = 2.0 * d_tx * c.inv_c;                                              // :215
    // (g + v_f tau_a) - (pos + vel tau_a) = d - v_rel tau_a (:216-218), so
    // d_rx^2 = d_tx^2 (1 - e), e = tau_a (2 d.w - tau_a |w|^2) / d_tx^2 ~ 1e-4: sqrt(1 - e) by its series
    // (e^5 / d_tx < 1e-20 relative; a second fp64 square root costs three times as much)
    const double eps = tau_a * (2.0 * dw - tau_a * w2) * (inv_d * inv_d);
    const double sq = fma(eps, fma(eps, fma(eps, fma(eps, -5.0 / 128.0, -1.0 / 16.0), -1.0 / 8.0), -0.5), 1.0);
    const double d_rx = d_tx * sq;
    const double tau = (d_tx + d_rx) * c.inv_c;                                             // :219
    const double idx_f = (tau - c.t_start + t_shift) * c.fs;                                // :221
    const float xn = (float)(2.0 * (idx_f * c.inv_ns) - 1.0);                               // :222, .float() :226
    tdbp_sample(c, xn, tau, p, acc_re, acc_im);
}

// ------------------------------------------------------------------------------------------------------------
// The same sum with the geometry expanded about the tile's reference pixel (round 5).  A 16 x 16 tile spans ~10 m at
// ranges of hundreds of kilometres, so per (tile, pulse) everything that needs a square root or a division is computed
// ONCE - by one lane per pulse, 256 pulses per batch, handed to the tile through LDS - and a pixel keeps only
//   d_tx = d0 sqrt(1 + u),  u = (2 D.q + |q|^2) / d0^2        as d0 (1 + u/2 - u^2/8 + u^3/16)   (u <= 5e-5: next term 5 u^4 / 128)
//   d_tx - d_rx = E0 + grad E . q                             (E = d_tx (1 - sqrt(1 + 4|w|^2/c^2 - 4 r / c)), r = d.w / d_tx: its
//                                                              leading term (2/c) d.w is exactly linear in q, the rest < 1e-11 m)
//   t_shift fs = ts0 + grad ts . q                            (fp32: it only moves the interpolation coordinate, by < 1e-6 sample)
// with q the pixel's offset from the reference pixel (exact differences of the axis tables).  22 fp64 instructions per
// pixel and pulse instead of 48; the launcher takes this form only when 5 u_max^4 / 128 * d_max < 1e-9 m over all
// pulses (tdbp_tile_ok), otherwise the exact one above.  Same pulse order per pixel and the same fp64 accumulation.
// ------------------------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) TilePulse {
    double a1, a2;           // 2 Dx, 2 Dy
    double inv_d0sq, d0;
    double e0, ex;
    double ey; float ts0, tsx;
    float tsy, pad0; double pad1;
};
static_assert(sizeof(TilePulse) == 80, "five 16-byte LDS reads per pulse");
static constexpr int TP_BATCH = 256;

// the record of one pulse: d and w as in the exact form, taken at the tile's reference pixel
template <class A> __device__ __forceinline__ TilePulse tdbp_tile_prologue(const A& c, double dx, double dy, double dz, double wx,
                                                                          double wy, double wz, double w2) {
    const double s0 = fma(dx, dx, fma(dy, dy, dz * dz));
    const double inv_d = rsqrt(s0), d0 = s0 * inv_d;
    const double dw = wx * dx + wy * dy + wz * dz;
    const double r = dw * inv_d;                                                            // :210-212
    const double tau_a = 2.0 * d0 * c.inv_c;
    const double eps = tau_a * (2.0 * dw - tau_a * w2) * (inv_d * inv_d);
    const double sm1 = eps * fma(eps, fma(eps, fma(eps, -5.0 / 128.0, -1.0 / 16.0), -1.0 / 8.0), -0.5);   // sqrt(1 - eps) - 1
    const double ux = dx * inv_d, uy = dy * inv_d;                                          // unit vector, ground components
    const double f = -sm1, fp = 2.0 * c.inv_c / (1.0 + sm1);                                // F(r) and F'(r)
    const double rx = (wx - r * ux) * inv_d, ry = (wy - r * uy) * inv_d;                    // grad r
    TilePulse t;
    t.a1 = 2.0 * dx; t.a2 = 2.0 * dy; t.inv_d0sq = inv_d * inv_d; t.d0 = d0;
    t.e0 = d0 * f;
    t.ex = fma(d0 * fp, rx, f * ux); t.ey = fma(d0 * fp, ry, f * uy);
    const double ks = c.k_shift * c.fs;
    t.ts0 = (float)(r * ks); t.tsx = (float)(rx * ks); t.tsy = (float)(ry * ks);
    t.pad0 = 0.f; t.pad1 = 0.0;
    return t;
}

// q: the pixel's offset from the reference pixel, q2 = |q|^2, qxf, qyf = (float)q; two_inv_ns = 2 / n_s
template <class A> __device__ __forceinline__ void tdbp_tile_pixel(const A& c, const TilePulse& t, double qx, double qy, double q2,
                                                                  float qxf, float qyf, double two_inv_ns, int p, double& acc_re,
                                                                  double& acc_im) {
    const double u = fma(t.a1, qx, fma(t.a2, qy, q2)) * t.inv_d0sq;
    const double h = u * fma(u, fma(u, 1.0 / 16.0, -1.0 / 8.0), 0.5);
    const double d_tx = fma(t.d0, h, t.d0);
    const double e = fma(t.ex, qx, fma(t.ey, qy, t.e0));                                    // d_tx - d_rx
    const double tau = fma(2.0, d_tx, -e) * c.inv_c;                                        // :219
    const float ts = fmaf(t.tsx, qxf, fmaf(t.tsy, qyf, t.ts0));                             // t_shift * fs (:213)
    const double idx_f = fma(tau - c.t_start, c.fs, (double)ts);                            // :221
    const float xn = (float)fma(idx_f, two_inv_ns, -1.0);                                   // :222, .float() :226
    tdbp_sample(c, xn, tau, p, acc_re, acc_im);
}

// ------------------------------------------------------------------------------------------------------------
// N = 2, 3 or 4 receivers (tdbp_multi.hip; N = 2 is the two-receiver pair and its search, 4.19): receiver c
// rides at pos_tx + off_c v^ (sar_ati_dcpa_sim_csa.py:145-159), there is no stop-and-go receiver and no t_shift.  d, s_tx, inv_d, d_tx
// are the transmit leg, computed once per pixel and pulse for every channel; dv = d . v^.
//   d_rx^2 = d_tx^2 - 2 off dv + off^2 = d_tx^2 (1 - e),  e = off (2 dv - off) / d_tx^2,  |e| <= 2 |off| / d_tx + (off / d_tx)^2.
// SERIES: sqrt(1 - e) by the series of tdbp_exact_pixel; its first omitted term is 7 e^5 / 256, and the launcher takes this form
// only when 7 e_max^5 / 256 * d_max < 1e-9 m over all pulses (tdbp_pair_bounds: e ~ 5e-6 at the reference geometry, where the
// term is 1e-23 m); otherwise the plain square root runs.
// A: the kernel's arguments, an RxArgs; PairChan: what tdbp_sample reads of one channel, made of the arguments per channel.
// ------------------------------------------------------------------------------------------------------------
static constexpr int MAX_RX = 4;

struct PairChan {
    const cf* rc;            // [n_p][n_s] range-compressed pulses of this channel
    double fc;
    float half_w;
    int n_s;
};

struct PairGeo {             // the receivers' table: one 64-byte record per pulse, read with scalar loads
    double px, py, pz;       // transmitter
    double ux, uy, uz;       // v^ = vel_tx / |vel_tx|
    double dt, pad;
};

// What the loops below read of a kernel's arguments: MultiArgs (tdbp_multi.hip) and PairSearchArgs (tdbp_pair_search.hip) derive from
// it, tdbp_rx_fill_args (tdbp_plan.h) sets it.  The order of the fields is kept as it is on purpose: with off[] ahead of the five
// constants the compiler gives the N = 2 tile kernel another schedule and register count.
struct RxArgs {
    const cf* rc[MAX_RX];    // [n_p][n_s] range-compressed pulses of channel c
    double fc;               // what tdbp_sample reads beside rc, the same for every channel
    float half_w;
    int n_s;
    const PairGeo* geo;
    double inv_c, fs, t_start, chirp_centre, inv_ns;
    double off[MAX_RX];
    int first[MAX_RX], n_used;   // channel c: pulses [first[c], first[c] + n_used)
    int u0, u1;              // their union
};

template <bool SERIES, class A> __device__ __forceinline__ void tdbp_pair_pixel(const A& c, const PairChan& ch, double s_tx, double inv_d,
                                                                              double d_tx, double dv, double off, int p, double& acc_re,
                                                                              double& acc_im) {
    double d_rx;
    if (SERIES) {
        const double eps = off * (2.0 * dv - off) * (inv_d * inv_d);
        const double sq = fma(eps, fma(eps, fma(eps, fma(eps, -5.0 / 128.0, -1.0 / 16.0), -1.0 / 8.0), -0.5), 1.0);
        d_rx = d_tx * sq;
    } else {
        d_rx = sqrt(fma(off, off - 2.0 * dv, s_tx));
    }
    const double tau = (d_tx + d_rx) * c.inv_c;
    const double idx_f = (tau - c.t_start + c.chirp_centre) * c.fs;
    const float xn = (float)(2.0 * (idx_f * c.inv_ns) - 1.0);
    tdbp_sample(ch, xn, tau, p, acc_re, acc_im);
}

// The pulses [p0, p1) of one pixel at (gx0, gy0) under the focus velocity vf, every channel.  A channel accumulates only inside its
// own pulse range (a wave-uniform test).
template <int N, bool SERIES, class A> __device__ __forceinline__ void tdbp_multi_pulses(const A& a, double vfx, double vfy, double vfz, double gx0,
                                                                                        double gy0, int p0, int p1, double (&re)[N], double (&im)[N]) {
    for (int p = p0; p < p1; ++p) {
        const PairGeo g = a.geo[p];
        const double dx = fma(vfx, g.dt, gx0) - g.px;
        const double dy = fma(vfy, g.dt, gy0) - g.py;
        const double dz = vfz * g.dt - g.pz;
        const double s_tx = fma(dx, dx, fma(dy, dy, dz * dz));
        const double inv_d = rsqrt(s_tx);                                                   // one reciprocal square root
        const double d_tx = s_tx * inv_d;                                                   // for every channel
        const double dv = g.ux * dx + g.uy * dy + g.uz * dz;
#pragma unroll
        for (int c = 0; c < N; ++c)
            if (p >= a.first[c] && p < a.first[c] + a.n_used) {
                const PairChan ch = {a.rc[c], a.fc, a.half_w, a.n_s};
                tdbp_pair_pixel<SERIES>(a, ch, s_tx, inv_d, d_tx, dv, a.off[c], p, re[c], im[c]);
            }
    }
}

// The same with the geometry expanded about the tile's reference pixel, as tdbp_tile_prologue / tdbp_tile_pixel do it: per
// (tile, pulse) one lane computes, with D the vector from the transmitter to the reference pixel and q the pixel's offset from it,
//   d_tx = d0 sqrt(1 + u),  u = (2 D.q + |q|^2) / d0^2            as d0 (1 + u/2 - u^2/8 + u^3/16), the series of tdbp_tile_pixel
//   d_tx - d_rx(c) = E_c0 + grad E_c . q                          E_c0 = off (2 D.v^ - off) / (d0 + d_rx0) (no cancellation),
//                                                                 grad E_c = u^_tx - u^_rx = (off d0 v^ - E_c0 D) / (d0 d_rx0)
// The remainder of the second line is q^T (H(d) - H(d - off v^)) q / 2 with H the Hessian of the Euclidean norm; the third
// derivative of the norm at x applied to (h, h, k), unit h and k, is (-(1 - a^2) b - 2 a h_perp . k_perp) / |x|^2 with a = h . x^,
// b = k . x^, whose modulus is at most sqrt((1 - a^2)(1 + 3 a^2)) <= 2 / sqrt(3).  So |remainder| <= |q|^2 |off| / (sqrt(3) d^2),
// d the nearest range less |off|; the launcher takes this form only when that and the d_tx series' omitted term both stay below
// 1e-9 m over all pulses and every channel (tdbp_tile_ok, tdbp_pair_bounds), otherwise the exact form above.

// the tile form's record: 32 + 24 N bytes, padded to a multiple of 16 (80, 112, 128)
template <int N> struct __attribute__((aligned(16))) MultiTilePulse {
    double a1, a2;           // 2 Dx, 2 Dy
    double inv_d0sq, d0;
    double e0[N], ex[N], ey[N];
};
static_assert(sizeof(MultiTilePulse<2>) == 80 && sizeof(MultiTilePulse<3>) == 112 && sizeof(MultiTilePulse<4>) == 128, "whole 16-byte LDS reads");

template <int N> __device__ __forceinline__ MultiTilePulse<N> tdbp_multi_tile_prologue(double dx, double dy, double dz, double ux, double uy, double uz,
                                                                                     const double* off) {
    const double s0 = fma(dx, dx, fma(dy, dy, dz * dz));
    const double inv_d = rsqrt(s0), d0 = s0 * inv_d;
    const double dv = ux * dx + uy * dy + uz * dz;
    MultiTilePulse<N> t;
    t.a1 = 2.0 * dx; t.a2 = 2.0 * dy; t.inv_d0sq = inv_d * inv_d; t.d0 = d0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const double d_rx = sqrt(fma(off[c], off[c] - 2.0 * dv, s0));
        const double e0 = off[c] * (2.0 * dv - off[c]) / (d0 + d_rx);
        const double inv = 1.0 / (d0 * d_rx);
        t.e0[c] = e0;
        t.ex[c] = (off[c] * d0 * ux - e0 * dx) * inv;
        t.ey[c] = (off[c] * d0 * uy - e0 * dy) * inv;
    }
    return t;
}

// d_tx of one pixel and pulse, for every channel.  T: MultiTilePulse<N>
template <class T> __device__ __forceinline__ double tdbp_pair_tile_dtx(const T& t, double qx, double qy, double q2) {
    const double u = fma(t.a1, qx, fma(t.a2, qy, q2)) * t.inv_d0sq;
    const double h = u * fma(u, fma(u, 1.0 / 16.0, -1.0 / 8.0), 0.5);
    return fma(t.d0, h, t.d0);
}

template <class A, class T> __device__ __forceinline__ void tdbp_pair_tile_pixel(const A& c, const PairChan& ch, const T& t, int chan,
                                                                      double d_tx, double qx, double qy, double two_inv_ns, int p,
                                                                      double& acc_re, double& acc_im) {
    const double e = fma(t.ex[chan], qx, fma(t.ey[chan], qy, t.e0[chan]));                  // d_tx - d_rx
    const double tau = fma(2.0, d_tx, -e) * c.inv_c;
    const double idx_f = (tau - c.t_start + c.chirp_centre) * c.fs;
    const float xn = (float)fma(idx_f, two_inv_ns, -1.0);
    tdbp_sample(ch, xn, tau, p, acc_re, acc_im);
}

// The pulses [p0, p1) in the tile form: one lane per pulse fills the batch's records s_tp [TP_BATCH] in LDS, then every pixel walks
// them.  Every thread of the workgroup comes here, dead lanes too: the loop holds two barriers per batch.
template <int N, class A> __device__ __forceinline__ void tdbp_multi_tile_pulses(const A& a, MultiTilePulse<N>* s_tp, double vfx, double vfy, double vfz,
                                                                               const TdbpTileOffsets& o, int p0, int p1, double (&re)[N], double (&im)[N]) {
    const double two_inv_ns = 2.0 * a.inv_ns;
    for (int pb = p0; pb < p1; pb += TP_BATCH) {
        const int nb = min(TP_BATCH, p1 - pb);
        __syncthreads();                                   // the previous batch has been consumed
        if ((int)threadIdx.x < nb) {
            const PairGeo g = a.geo[pb + threadIdx.x];
            const double dx = fma(vfx, g.dt, o.xc) - g.px, dy = fma(vfy, g.dt, o.yc) - g.py, dz = vfz * g.dt - g.pz;
            s_tp[threadIdx.x] = tdbp_multi_tile_prologue<N>(dx, dy, dz, g.ux, g.uy, g.uz, a.off);
        }
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
            const int p = pb + k;
            const double d_tx = tdbp_pair_tile_dtx(s_tp[k], o.qx, o.qy, o.q2);
#pragma unroll
            for (int c = 0; c < N; ++c)
                if (p >= a.first[c] && p < a.first[c] + a.n_used) {
                    const PairChan ch = {a.rc[c], a.fc, a.half_w, a.n_s};
                    tdbp_pair_tile_pixel(a, ch, s_tp[k], c, d_tx, o.qx, o.qy, two_inv_ns, p, re[c], im[c]);
                }
        }
    }
}

}  // namespace sarx
