// Two-channel balance (include/sarx_balance.h): block sums of slc1 conj(slc2), |slc1|^2, |slc2|^2 over both images, a complex
// weight and a coherence per block, and the launch that multiplies channel 2 by the interpolated weight.
//
// Estimate: a block is cut into strips of BAL_STRIP_ROWS rows x the block's width; one workgroup reduces one strip.  A strip's
// pixels are taken in pairs (columns 2q, 2q + 1 of the block); pair e = row * pairs_per_row + q belongs to thread e % 256 and a
// thread adds its pairs in rising e, so which thread adds what, and in which order, follows from the shapes alone.  A
// pair arrives as one 16-byte load per image when every pair of the call starts on a 16-byte boundary (even n_rg and block_rg,
// images 16-byte aligned: the VEC instantiation, chosen on the host), otherwise as two 8-byte loads: the addresses decide how
// the bytes arrive, never where they are added.  Four pairs per thread (eight loads with VEC) are issued before the first is
// used.  fp64 per thread, then a shuffle reduction per wave, then the four waves through
// LDS in wave order; the strip's sums go to the workspace.  Weights: one workgroup adds each block's strips in strip order,
// writes the record, reduces the valid blocks' sums (per thread in block order, waves by shuffles, waves in order) and hands the
// global weight to the blocks that are not valid.  No atomics anywhere.
//
// Apply: one workgroup per 16 rows x 512 columns.  The weights of the (at most 4 x 66) blocks the tile touches go to LDS as fp32,
// are interpolated along azimuth once per tile row, and each thread interpolates along range for the two columns it owns.  A
// thread loads its pixels of four rows (16 bytes per image and row in the VEC instantiation, as above), then writes them: each
// pixel is read and written by one thread only, so slc2_out may be slc2.
#include "balance.h"

namespace sarx {

typedef float2 cf;

static constexpr int BAL_THREADS = 256, BAL_UNROLL = 4;
static constexpr int BAL_W_THREADS = 1024;
static constexpr int AP_ROWS = 16, AP_COLS = 512, AP_BR = 4, AP_BC = 68, AP_UNROLL = 4;

// pixels p[0] and (two) p[1].  VEC: the caller has shown that p is 16-byte aligned and that both pixels exist
template <bool VEC> __device__ __forceinline__ void load_pair(const cf* p, bool two, cf& x0, cf& x1) {
    if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        x0 = make_float2(v.x, v.y);
        x1 = make_float2(v.z, v.w);
    } else {
        x0 = p[0];
        x1 = two ? p[1] : make_float2(0.f, 0.f);
    }
}

struct BalSums {
    double s12_re, s12_im, s11, s22;
    unsigned long long n;
};

__device__ __forceinline__ void bal_add(cf a, cf b, bool valid, float clip, BalSums& s) {
    const float p1 = fmaf(a.x, a.x, __fmul_rn(a.y, a.y)), p2 = fmaf(b.x, b.x, __fmul_rn(b.y, b.y));
    const bool keep = valid && p1 <= clip && p2 <= clip;              // NaN: not kept
    const double ax = keep ? (double)a.x : 0.0, ay = keep ? (double)a.y : 0.0;
    const double bx = keep ? (double)b.x : 0.0, by = keep ? (double)b.y : 0.0;
    s.s12_re = fma(ax, bx, s.s12_re); s.s12_re = fma(ay, by, s.s12_re);      // a conj(b); every product is exact in fp64
    s.s12_im = fma(ay, bx, s.s12_im); s.s12_im = fma(-ax, by, s.s12_im);
    s.s11 = fma(ax, ax, s.s11); s.s11 = fma(ay, ay, s.s11);
    s.s22 = fma(bx, bx, s.s22); s.s22 = fma(by, by, s.s22);
    s.n += keep ? 1u : 0u;
}

__device__ __forceinline__ void wave_sum(BalSums& s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s.s12_re += __shfl_down(s.s12_re, off);
        s.s12_im += __shfl_down(s.s12_im, off);
        s.s11 += __shfl_down(s.s11, off);
        s.s22 += __shfl_down(s.s22, off);
        s.n += __shfl_down(s.n, off);
    }
}

template <bool VEC> __global__ __launch_bounds__(BAL_THREADS) void balance_estimate_kernel(BalanceEstimateArgs a) {
    __shared__ BalSums red[BAL_THREADS / 64];
    const BalanceGeom g = a.g;
    const int tid = threadIdx.x;
    const unsigned sid = blockIdx.x;
    const int strip = sid % g.strips;
    const unsigned b = sid / g.strips;
    const int br = b % g.nb_rg, ba = b / g.nb_rg;
    const int j0 = br * g.block_rg, W = min(g.block_rg, g.n_rg - j0);
    const int i0 = ba * g.block_az + strip * BAL_STRIP_ROWS;
    const int i1 = min(min((ba + 1) * g.block_az, g.n_az), i0 + BAL_STRIP_ROWS);
    const int R = max(i1 - i0, 0);                                   // a ragged block's last strips are empty
    const int SP = (W + 1) >> 1;                                     // pairs per row
    const int total = R * SP;
    const size_t first = (size_t)min(i0, g.n_az - 1) * g.n_rg + j0;  // a pixel that exists: what a slot past the end loads (and drops)
    BalSums s{0.0, 0.0, 0.0, 0.0, 0ull};
    int r = tid / SP, q = tid - r * SP;                              // pair e = tid, then + 256 per step
    const int dr = BAL_THREADS / SP, dq = BAL_THREADS - dr * SP;
    for (int it = 0; it < total; it += BAL_THREADS * BAL_UNROLL) {
        cf A0[BAL_UNROLL], A1[BAL_UNROLL], B0[BAL_UNROLL], B1[BAL_UNROLL];
        bool ok[BAL_UNROLL], two[BAL_UNROLL];
#pragma unroll
        for (int u = 0; u < BAL_UNROLL; ++u) {
            ok[u] = it + u * BAL_THREADS + tid < total;
            two[u] = ok[u] && 2 * q + 1 < W;
            const size_t idx = ok[u] ? (size_t)(i0 + r) * g.n_rg + j0 + 2 * q : first;
            load_pair<VEC>(a.s1 + idx, two[u], A0[u], A1[u]);
            load_pair<VEC>(a.s2 + idx, two[u], B0[u], B1[u]);
            r += dr; q += dq;
            if (q >= SP) { q -= SP; ++r; }
        }
#pragma unroll
        for (int u = 0; u < BAL_UNROLL; ++u) {
            bal_add(A0[u], B0[u], ok[u], a.clip, s);
            bal_add(A1[u], B1[u], two[u], a.clip, s);
        }
    }
    wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        BalSums t = red[0];
#pragma unroll
        for (int w = 1; w < BAL_THREADS / 64; ++w) {
            t.s12_re += red[w].s12_re; t.s12_im += red[w].s12_im; t.s11 += red[w].s11; t.s22 += red[w].s22; t.n += red[w].n;
        }
        BalPartial p;
        p.s12_re = t.s12_re; p.s12_im = t.s12_im; p.s11 = t.s11; p.s22 = t.s22; p.n = t.n;
        a.part[sid] = p;
    }
}

// weight and coherence of one set of sums (a block's, or the valid blocks' together)
__device__ __forceinline__ bool bal_weight(double s12_re, double s12_im, double s11, double s22, int mode, double& w_re, double& w_im,
                                           double& coh) {
    const double m = hypot(s12_re, s12_im);
    const double d = s11 * s22;
    coh = d > 0.0 ? m / sqrt(d) : 0.0;
    if (!(s22 > 0.0) || !(m > 0.0)) { w_re = 1.0; w_im = 0.0; return false; }
    const double den = mode == SARX_BALANCE_PHASE ? m : s22;
    w_re = s12_re / den;
    w_im = s12_im / den;
    return true;
}

__global__ __launch_bounds__(BAL_W_THREADS) void balance_weights_kernel(BalanceEstimateArgs a) {
    constexpr int WAVES = BAL_W_THREADS / 64;
    __shared__ BalSums red[WAVES];
    __shared__ unsigned red_valid[WAVES];
    __shared__ double gw[2];
    const BalanceGeom g = a.g;
    const int tid = threadIdx.x;
    const int nblocks = g.nb_az * g.nb_rg;
    BalSums s{0.0, 0.0, 0.0, 0.0, 0ull};
    unsigned n_valid = 0;
    for (int b = tid; b < nblocks; b += BAL_W_THREADS) {
        const BalPartial* p = a.part + (size_t)b * g.strips;
        BalSums t{0.0, 0.0, 0.0, 0.0, 0ull};
        for (int k = 0; k < g.strips; ++k) {
            t.s12_re += p[k].s12_re; t.s12_im += p[k].s12_im; t.s11 += p[k].s11; t.s22 += p[k].s22; t.n += p[k].n;
        }
        double w_re, w_im, coh;
        bool valid = bal_weight(t.s12_re, t.s12_im, t.s11, t.s22, a.mode, w_re, w_im, coh);
        valid = valid && t.n >= (unsigned long long)a.min_count && coh >= a.min_coherence;
        sarx_balance_record rec;
        rec.s12_re = t.s12_re; rec.s12_im = t.s12_im; rec.s11 = t.s11; rec.s22 = t.s22;
        rec.w_re = w_re; rec.w_im = w_im;                             // replaced below when the block is not valid
        rec.coherence = (float)coh;
        rec.n = (uint32_t)t.n;
        rec.valid = valid ? 1u : 0u;
        rec.reserved = 0u;
        a.rec[b] = rec;
        if (valid) {
            s.s12_re += t.s12_re; s.s12_im += t.s12_im; s.s11 += t.s11; s.s22 += t.s22; s.n += t.n;
            ++n_valid;
        }
    }
    wave_sum(s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_valid += __shfl_down(n_valid, off);
    if ((tid & 63) == 0) { red[tid >> 6] = s; red_valid[tid >> 6] = n_valid; }
    __syncthreads();
    if (tid == 0) {
        BalSums t = red[0];
        unsigned nv = red_valid[0];
        for (int w = 1; w < WAVES; ++w) {
            t.s12_re += red[w].s12_re; t.s12_im += red[w].s12_im; t.s11 += red[w].s11; t.s22 += red[w].s22; t.n += red[w].n;
            nv += red_valid[w];
        }
        double w_re = 1.0, w_im = 0.0, coh = 0.0;
        if (nv == 0 || !bal_weight(t.s12_re, t.s12_im, t.s11, t.s22, a.mode, w_re, w_im, coh)) {
            w_re = 1.0; w_im = 0.0; nv = 0;
        }
        sarx_balance_header h;
        h.nb_az = (uint32_t)g.nb_az; h.nb_rg = (uint32_t)g.nb_rg; h.n_valid = nv; h.reserved = 0u;
        h.w_re = w_re; h.w_im = w_im; h.coherence = coh;
        h.s11 = t.s11; h.s22 = t.s22; h.n = t.n;
        *a.hdr = h;
        gw[0] = w_re; gw[1] = w_im;
    }
    __syncthreads();
    const double g_re = gw[0], g_im = gw[1];
    for (int b = tid; b < nblocks; b += BAL_W_THREADS)                // the records this thread wrote above
        if (!a.rec[b].valid) { a.rec[b].w_re = g_re; a.rec[b].w_im = g_im; }
}

hipError_t launch_balance_estimate(const BalanceEstimateArgs& a, hipStream_t st) {
    const unsigned strips = (unsigned)a.g.nb_az * a.g.nb_rg * a.g.strips;
    // every pair of every block starts on a 16-byte boundary and is whole
    const bool vec = a.g.n_rg % 2 == 0 && a.g.block_rg % 2 == 0 && (((uintptr_t)a.s1 | (uintptr_t)a.s2) & 15) == 0;
    if (vec) hipLaunchKernelGGL(balance_estimate_kernel<true>, dim3(strips), dim3(BAL_THREADS), 0, st, a);
    else hipLaunchKernelGGL(balance_estimate_kernel<false>, dim3(strips), dim3(BAL_THREADS), 0, st, a);
    hipLaunchKernelGGL(balance_weights_kernel, dim3(1), dim3(BAL_W_THREADS), 0, st, a);
    return hipGetLastError();
}

// index i of an axis cut into nb blocks of `block`: the two block indices it interpolates between and the fraction of the second.
// t = (2 i + 1 - block) / (2 block) in integers, so f carries one fp32 rounding whatever the image size
__device__ __forceinline__ void bal_axis(int i, int block, int nb, int interp, int& b0, int& b1, float& f) {
    if (interp == SARX_BALANCE_NEAREST) { b0 = b1 = i / block; f = 0.f; return; }
    const int u = 2 * i + 1 - block;
    if (u <= 0) { b0 = 0; f = 0.f; }
    else { b0 = u / (2 * block); f = (float)(u - b0 * 2 * block) / (float)(2 * block); }
    const int top = max(nb - 2, 0);
    if (b0 > top) { b0 = top; f = nb >= 2 ? 1.f : 0.f; }             // past the last centre: constant
    b1 = min(b0 + 1, nb - 1);
}

__device__ __forceinline__ cf lerp2(cf x, cf y, float f) {
    const float e = 1.f - f;
    return make_float2(e * x.x + f * y.x, e * x.y + f * y.y);
}

template <bool DM, bool VEC> __global__ __launch_bounds__(BAL_THREADS) void balance_apply_kernel(BalanceApplyArgs a) {
    __shared__ cf raw[AP_BR][AP_BC];
    __shared__ cf wr[AP_ROWS][AP_BC];
    const BalanceGeom g = a.g;
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * AP_COLS, r0 = blockIdx.y * AP_ROWS;
    const int rows = min(AP_ROWS, g.n_az - r0), cols = min(AP_COLS, g.n_rg - c0);
    int ba_lo, bc_lo, t1;
    float tf;
    bal_axis(r0, g.block_az, g.nb_az, a.interp, ba_lo, t1, tf);
    bal_axis(c0, g.block_rg, g.nb_rg, a.interp, bc_lo, t1, tf);
    for (int e = tid; e < AP_BR * AP_BC; e += BAL_THREADS) {
        const int rr = e / AP_BC, cc = e - rr * AP_BC;
        const sarx_balance_record* rec = a.rec + (size_t)min(ba_lo + rr, g.nb_az - 1) * g.nb_rg + min(bc_lo + cc, g.nb_rg - 1);
        raw[rr][cc] = make_float2((float)rec->w_re, (float)rec->w_im);
    }
    __syncthreads();
    for (int e = tid; e < AP_ROWS * AP_BC; e += BAL_THREADS) {
        const int rr = e / AP_BC, cc = e - rr * AP_BC;
        int b0, b1;
        float f;
        bal_axis(min(r0 + rr, g.n_az - 1), g.block_az, g.nb_az, a.interp, b0, b1, f);
        wr[rr][cc] = lerp2(raw[min(b0 - ba_lo, AP_BR - 1)][cc], raw[min(b1 - ba_lo, AP_BR - 1)][cc], f);
    }
    __syncthreads();

    const int c = 2 * tid;                                           // this thread's columns of the tile: c, c + 1
    if (c >= cols) return;
    const bool two = c + 1 < cols;
    int k0[2], k1[2];
    float fr[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        int b0, b1;
        bal_axis(min(c0 + c + x, g.n_rg - 1), g.block_rg, g.nb_rg, a.interp, b0, b1, fr[x]);
        k0[x] = min(b0 - bc_lo, AP_BC - 1);
        k1[x] = min(b1 - bc_lo, AP_BC - 1);
    }
    for (int rb = 0; rb < rows; rb += AP_UNROLL) {
        cf X0[AP_UNROLL], X1[AP_UNROLL], Y0[AP_UNROLL], Y1[AP_UNROLL];
#pragma unroll
        for (int u = 0; u < AP_UNROLL; ++u) {                        // every load of the four rows before their first store
            const size_t idx = (size_t)(r0 + min(rb + u, rows - 1)) * g.n_rg + c0 + c;
            load_pair<VEC>(a.s2 + idx, two, X0[u], X1[u]);
            if (DM) load_pair<VEC>(a.s1 + idx, two, Y0[u], Y1[u]);
        }
#pragma unroll
        for (int u = 0; u < AP_UNROLL; ++u) {
            if (rb + u >= rows) break;
            const int rr = rb + u;
            const size_t idx = (size_t)(r0 + rr) * g.n_rg + c0 + c;
            const cf w0 = lerp2(wr[rr][k0[0]], wr[rr][k1[0]], fr[0]);
            const cf w1 = lerp2(wr[rr][k0[1]], wr[rr][k1[1]], fr[1]);
            const cf o0 = make_float2(fmaf(w0.x, X0[u].x, -w0.y * X0[u].y), fmaf(w0.x, X0[u].y, w0.y * X0[u].x));
            const cf o1 = make_float2(fmaf(w1.x, X1[u].x, -w1.y * X1[u].y), fmaf(w1.x, X1[u].y, w1.y * X1[u].x));
            cf* po = a.out + idx;
            if (VEC) {
                *reinterpret_cast<float4*>(po) = make_float4(o0.x, o0.y, o1.x, o1.y);
            } else {
                po[0] = o0;
                if (two) po[1] = o1;
            }
            if (DM) {
                const float d0 = hypotf(Y0[u].x - o0.x, Y0[u].y - o0.y), d1 = hypotf(Y1[u].x - o1.x, Y1[u].y - o1.y);
                float* pd = a.dm + idx;
                if (VEC) {
                    *reinterpret_cast<float2*>(pd) = make_float2(d0, d1);
                } else {
                    pd[0] = d0;
                    if (two) pd[1] = d1;
                }
            }
        }
    }
}

hipError_t launch_balance_apply(const BalanceApplyArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.g.n_rg + AP_COLS - 1) / AP_COLS), (unsigned)((a.g.n_az + AP_ROWS - 1) / AP_ROWS));
    // even rows of 16-byte aligned images (and an 8-byte aligned plane): every pair of a tile is whole and aligned
    const bool vec = a.g.n_rg % 2 == 0 && (((uintptr_t)a.s1 | (uintptr_t)a.s2 | (uintptr_t)a.out) & 15) == 0 && ((uintptr_t)a.dm & 7) == 0;
    if (a.dm) {
        if (vec) hipLaunchKernelGGL((balance_apply_kernel<true, true>), grid, dim3(BAL_THREADS), 0, st, a);
        else hipLaunchKernelGGL((balance_apply_kernel<true, false>), grid, dim3(BAL_THREADS), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((balance_apply_kernel<false, true>), grid, dim3(BAL_THREADS), 0, st, a);
        else hipLaunchKernelGGL((balance_apply_kernel<false, false>), grid, dim3(BAL_THREADS), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace sarx
