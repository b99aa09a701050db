// Wave-private azimuth tiles for 128-point column transforms (both steps of the 16384-point four-step transform).
//
// One wave owns one whole [128 rows x 32 columns] tile in registers: lane l < 32 holds column l, rows 0..63; lane l + 32
// the same column, rows 64..127 (64 complex points, 128 VGPRs of data per lane).  No LDS, no s_barrier, no dependency
// between waves: a wave that computes does not hold back another wave's loads (az_tile_kernel exchanges its radix-16 /
// radix-8 stages through LDS between two workgroup barriers, and a workgroup at a barrier has no request in flight).
// Every load and store instruction touches one 256-byte row segment in each of two rows.
//
// Transform (decimation in frequency), n = n1 + 64 n2, k = 2 k1 + k2:
//   radix 2 over n2 (the two half-waves, exchanged by v_permlane32_swap), times W_128^(n1 k2), then a 64-point DFT over
//   n1 inside each lane (8 x 8, compile-time twiddles).  The lower half-wave ends with the even outputs k = 2 k1, the
//   upper with the odd ones.
// Epilogues and four-step addressing are those of az_tile_kernel (csa_kernels.hip) for TWIDDLE, PHI1 and SCALE.
#include "csa_kernels.h"
#include "fft_core.hpp"
#include "phase.hpp"

// SARX_AZ_WAVE_NOFFT=1: the same loads, epilogues and stores with the transform compiled out (a traffic-only build that
// times what the layout alone allows; never the product)
#ifndef SARX_AZ_WAVE_NOFFT
#define SARX_AZ_WAVE_NOFFT 0
#endif

namespace sarx {

namespace {

// cos / sin of 2 pi j / 128 from a quarter table (exact 0 and 1 at the quadrant points)
constexpr float QCOS[33] = {1.000000000e+00f, 9.987954562e-01f, 9.951847267e-01f, 9.891765100e-01f, 9.807852804e-01f, 9.700312532e-01f,
                            9.569403357e-01f, 9.415440652e-01f, 9.238795325e-01f, 9.039892931e-01f, 8.819212643e-01f, 8.577286100e-01f,
                            8.314696123e-01f, 8.032075315e-01f, 7.730104534e-01f, 7.409511254e-01f, 7.071067812e-01f, 6.715589548e-01f,
                            6.343932842e-01f, 5.956993045e-01f, 5.555702330e-01f, 5.141027442e-01f, 4.713967368e-01f, 4.275550934e-01f,
                            3.826834324e-01f, 3.368898534e-01f, 2.902846773e-01f, 2.429801799e-01f, 1.950903220e-01f, 1.467304745e-01f,
                            9.801714033e-02f, 4.906767433e-02f, 0.0f};
constexpr float cos128(int j) {
    j &= 127;
    return j <= 32 ? QCOS[j] : j <= 64 ? -QCOS[64 - j] : j <= 96 ? -QCOS[j - 64] : QCOS[128 - j];
}
constexpr float sin128(int j) { return cos128(j - 32); }

// x * W_128^j (W = exp(-2 pi i / 128) forward, its conjugate inverse); j is a constant once the caller's loops are unrolled
template <bool INV> __device__ __forceinline__ cf mul_w128(cf x, int j) {
    j &= 127;
    if (j == 0) return x;
    if (j == 32) return mul_mi<INV>(x);
    if (j == 64) return make_float2(-x.x, -x.y);
    if (j == 96) return mul_mi<!INV>(x);
    return cmul(x, make_float2(cos128(j), INV ? sin128(j) : -sin128(j)));
}

// 64-point DFT of v[0..63] in natural order, in place: n = a + 8 b, k = c + 8 d; DFT_8 over b, * W_64^(a c), DFT_8 over a
template <bool INV> __device__ __forceinline__ void dft64(cf* v) {
    cf y[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        cf t[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) t[b] = v[a + 8 * b];
        dft8<INV>(t);
#pragma unroll
        for (int c = 0; c < 8; ++c) y[a][c] = t[c];
    }
#pragma unroll
    for (int a = 1; a < 8; ++a)
#pragma unroll
        for (int c = 1; c < 8; ++c) y[a][c] = mul_w128<INV>(y[a][c], 2 * a * c);     // W_64^(a c)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        cf t[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) t[a] = y[a][c];
        dft8<INV>(t);
#pragma unroll
        for (int d = 0; d < 8; ++d) v[c + 8 * d] = t[d];
    }
}

// lower half-wave's v[2p + 1] <-> upper half-wave's v[2p], p < 32 (both floats of each)
__device__ __forceinline__ void swap_pairs(cf* v) {
#pragma unroll
    for (int p = 0; p < 32; ++p) {
        auto rx = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2 * p].x), __float_as_uint(v[2 * p + 1].x), false, false);
        auto ry = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2 * p].y), __float_as_uint(v[2 * p + 1].y), false, false);
        v[2 * p] = make_float2(__uint_as_float(rx[0]), __uint_as_float(ry[0]));
        v[2 * p + 1] = make_float2(__uint_as_float(rx[1]), __uint_as_float(ry[1]));
    }
}

// 128-point transform of the column held by a lane pair: in, v[i] = x[i + 64 h]; out, v[k1] = X[2 k1 + h]
template <bool INV> __device__ __forceinline__ void fft128_wave(cf* v, bool h) {
    // after the swap, lane half h holds (x[n1], x[n1 + 64]) of n1 = 2p + h in (v[2p], v[2p + 1])
    swap_pairs(v);
#pragma unroll
    for (int p = 0; p < 32; ++p) {
        const cf s = cadd(v[2 * p], v[2 * p + 1]);
        const cf d = csub(v[2 * p], v[2 * p + 1]);
        const int j0 = 2 * p, j1 = 2 * p + 1;                  // W_128^(n1): the exponent differs between the halves
        const float wc = h ? cos128(j1) : cos128(j0);
        const float ws = h ? sin128(j1) : sin128(j0);
        v[2 * p] = s;
        v[2 * p + 1] = cmul(d, make_float2(wc, INV ? ws : -ws));
    }
    // back: the lower half holds the sums (k2 = 0) of every n1, the upper half the twiddled differences (k2 = 1)
    swap_pairs(v);
    dft64<INV>(v);
}

__device__ __forceinline__ double readlane_d(double x, int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, l), hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double2 readlane_d2(double2 x, int l) { return make_double2(readlane_d(x.x, l), readlane_d(x.y, l)); }

}  // namespace

// WPB independent waves per workgroup, each on its own tile (adjacent 32-column groups of the same q)
template <bool INV, int EPI, bool NT, int WPB>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(2))) void az_wave_kernel(AzArgs a) {
    constexpr int H = 64;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const bool h = lane >= 32;
    const int col = (blockIdx.x * WPB + wave) * 32 + (lane & 31);
    const int q = blockIdx.y + a.q0;
    const size_t n_rg = (size_t)a.n_rg;

    const size_t out_base = (size_t)q * a.out_q_stride;
    // PHI1: the tile's 128 rows of c1, two per lane (rows m = lane, lane + 64), requested ahead of the image; the epilogue
    // reads a row's constants from its lane (a vector load per output row made the wave wait for each one in turn)
    double2 c1a = make_double2(0.0, 0.0), c1b = c1a;
    if constexpr (EPI == AZ_EPI_PHI1) {
        c1a = a.c1[out_base + (size_t)lane * a.out_m_stride];
        c1b = a.c1[out_base + (size_t)(lane + H) * a.out_m_stride];
    }
    cf v[H];
    {
        const cf* src = a.in + ((size_t)q * a.in_q_stride + (size_t)(h ? H : 0) * a.in_m_stride) * n_rg + col;
        const size_t step = (size_t)a.in_m_stride * n_rg;
#pragma unroll
        for (int i = 0; i < H; ++i) v[i] = ld8<NT>(src + i * step);
    }
    __builtin_amdgcn_sched_barrier(0);      // all 64 loads in flight before the first exchange waits for any of them
#if !SARX_AZ_WAVE_NOFFT
    fft128_wave<INV>(v, h);
#endif
    __builtin_amdgcn_sched_barrier(0);
    cf* dst = a.out + (out_base + (size_t)(h ? 1 : 0) * a.out_m_stride) * n_rg + col;
    const size_t ostep = 2 * (size_t)a.out_m_stride * n_rg;     // output k1 of this half is tile row m = 2 k1 + h
    float best2 = -1.f;
    cf best = make_float2(0.f, 0.f);
#pragma unroll
    for (int k1 = 0; k1 < H; ++k1) {
        const int m = 2 * k1 + (h ? 1 : 0);
        cf x = v[k1];
        if constexpr (EPI == AZ_EPI_TWIDDLE) {       // four-step twiddle W_n^(q m), exact fp32 argument (see az_tile_kernel)
            const float rev = (float)(q * m) * a.scale;
            x = cmul(x, cis_frac(INV ? rev : -rev));
        } else if constexpr (EPI == AZ_EPI_PHI1) {
            const double2& src = k1 < H / 2 ? c1a : c1b;     // rows 2 k1 (lower half) and 2 k1 + 1 (upper half)
            const double2 lo = readlane_d2(src, (2 * k1) & (H - 1)), hi = readlane_d2(src, (2 * k1 + 1) & (H - 1));
            x = cmul(x, phi1(col, h ? hi : lo, a.dt, a.t_start));
        } else if constexpr (EPI == AZ_EPI_SCALE) {
            x.x *= a.scale; x.y *= a.scale;
            // the sample of largest |x|^2 is kept and hypotf taken of it once: 64 inline hypotf spilled the kernel's registers
            const float p2 = fmaf(x.x, x.x, x.y * x.y);
            if (p2 > best2) { best2 = p2; best = x; }
        }
        st8<NT>(dst + k1 * ostep, x);
    }
    if constexpr (EPI == AZ_EPI_SCALE) {
        if (a.max_out) {       // sharded max |image| as in az_tile_kernel (a maximum: the same bits whatever the sharding)
            float vmax = hypotf(best.x, best.y);
            for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
            if (lane == 0)
                atomicMax(a.max_out + 32u * (((blockIdx.x * WPB + wave) * 7u + blockIdx.y * 13u) & (MAX_SHARDS - 1u)), __float_as_uint(vmax));
        }
    }
}

template <bool INV, int EPI, bool NT, int WPB> static hipError_t launch_wave_one(const AzArgs& a, int nq, hipStream_t st) {
    dim3 grid(a.n_rg / (32 * WPB), nq);
    hipLaunchKernelGGL((az_wave_kernel<INV, EPI, NT, WPB>), grid, dim3(64 * WPB), 0, st, a);
    return hipGetLastError();
}
template <bool INV, int EPI, bool NT> static hipError_t launch_wave_nt(int wpb, const AzArgs& a, int nq, hipStream_t st) {
    switch (wpb) {
        case 1: return launch_wave_one<INV, EPI, NT, 1>(a, nq, st);
        case 4: return launch_wave_one<INV, EPI, NT, 4>(a, nq, st);
    }
    return hipErrorInvalidValue;
}
template <bool INV, int EPI> static hipError_t launch_wave_epi(int wpb, const AzArgs& a, int nq, hipStream_t st) {
    return a.nt ? launch_wave_nt<INV, EPI, true>(wpb, a, nq, st) : launch_wave_nt<INV, EPI, false>(wpb, a, nq, st);
}

bool az_wave_supported(int r, int n_rg, int epi, int wpb) {
    return r == 128 && (wpb == 1 || wpb == 4) && n_rg % (32 * wpb) == 0 &&
           (epi == AZ_EPI_TWIDDLE || epi == AZ_EPI_PHI1 || epi == AZ_EPI_SCALE);
}

hipError_t launch_az_wave(bool inv, int epi, int wpb, const AzArgs& a, int nq, hipStream_t st) {
    if (!inv) {
        switch (epi) {
            case AZ_EPI_TWIDDLE: return launch_wave_epi<false, AZ_EPI_TWIDDLE>(wpb, a, nq, st);
            case AZ_EPI_PHI1: return launch_wave_epi<false, AZ_EPI_PHI1>(wpb, a, nq, st);
        }
    } else {
        switch (epi) {
            case AZ_EPI_TWIDDLE: return launch_wave_epi<true, AZ_EPI_TWIDDLE>(wpb, a, nq, st);
            case AZ_EPI_SCALE: return launch_wave_epi<true, AZ_EPI_SCALE>(wpb, a, nq, st);
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace sarx
