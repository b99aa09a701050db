// GMTI detection on the DPCA magnitude plane (include/sarx_gmti.h): a cell-averaging CFAR launch that appends the peaks of the
// detected cells to a list, and a refine launch that sorts the list by (i, j) and adds the ATI interferogram of each report.
//
// CFAR: one workgroup per tile of gmti_dev.hpp, which states the tile's geometry, the peak rule, the report and the ranks for
// this detector and for oscfar.hip.  The tile and its halo are read into LDS with range-direction (contiguous) loads,
// all issued before the first wait; outside the image the tile holds zeros.  Box sums of P = m^2 are separable and fp64
// throughout: a vertical pass writes per column the sums over the outer and the guard rows of each output row (running sums over
// eight output rows per thread), a horizontal pass slides the same two windows along each row.  The training sum is outer - guard:
// in fp64 the error of that difference is about 1e-16 of the largest P in the window, far inside the threshold's resolution even
// with a target 60 dB over the clutter (an fp32 prefix-sum difference is not).  Detected cells are tested against their guard box
// from LDS (the peak rule), and the reports are compacted with one atomic per wave (ballot + mbcnt prefix).  Nothing is written
// per cell.
#include "gmti.h"

#include <climits>

#include "gmti_dev.hpp"

namespace sarx {

static constexpr int GM_SEG = 8;              // output rows (vertical pass) / columns (horizontal pass) per running sum
static constexpr int REFINE_THREADS = 256;

template <int HA, int HR> __global__ __launch_bounds__(CFAR_THREADS) void gmti_cfar_kernel(GmtiCfarArgs a) {
    using Tile = CfarTile<HA, HR>;
    constexpr int LH = Tile::LH, LW = Tile::LW, K = Tile::K;
    constexpr int VW = LW + 1;                // odd row stride (doubles): the horizontal pass reads one column of 32 rows per half-wave
    __shared__ float tile[LH][LW];
    __shared__ double vo[CFAR_TH][VW], vg[CFAR_TH][VW];
    const int r0 = blockIdx.y * CFAR_TH, c0 = blockIdx.x * CFAR_TW;
    const int tid = threadIdx.x;

    // tile fill: every address is clamped into the image (always a valid load), the value outside it is replaced by zero afterwards,
    // so the K loads carry no branch and are issued back to back
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * CFAR_THREADS;
        const int gr = r0 - HA + e / LW, gc = c0 - HR + e % LW;
        const int cr = min(max(gr, 0), a.n_az - 1), cc = min(max(gc, 0), a.n_rg - 1);
        v[k] = a.m[(size_t)cr * a.n_rg + cc];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * CFAR_THREADS;
        const int gr = r0 - HA + e / LW, gc = c0 - HR + e % LW;
        const bool inside = (unsigned)gr < (unsigned)a.n_az && (unsigned)gc < (unsigned)a.n_rg;
        tile[e / LW][e % LW] = inside ? v[k] : 0.f;
    }
    __syncthreads();

    // vertical pass: column c of the tile, output rows [seg * 8, seg * 8 + 8)
    for (int item = tid; item < (CFAR_TH / GM_SEG) * LW; item += CFAR_THREADS) {
        const int c = item % LW, rb = (item / LW) * GM_SEG;
        const int lr = rb + HA;                                   // tile row of output row rb
        double so = 0.0, sg = 0.0;
        for (int d = -a.oa; d <= a.oa; ++d) { const double x = tile[lr + d][c]; so += x * x; }
        for (int d = -a.ga; d <= a.ga; ++d) { const double x = tile[lr + d][c]; sg += x * x; }
        vo[rb][c] = so;
        vg[rb][c] = sg;
        for (int q = 1; q < GM_SEG; ++q) {
            const int r = lr + q;
            const double ai = tile[r + a.oa][c], ao = tile[r - 1 - a.oa][c];
            const double gi = tile[r + a.ga][c], go = tile[r - 1 - a.ga][c];
            so += ai * ai; so -= ao * ao;
            sg += gi * gi; sg -= go * go;
            vo[rb + q][c] = so;
            vg[rb + q][c] = sg;
        }
    }
    __syncthreads();

    // horizontal pass: output row r, output columns [cb, cb + 8); threshold and peak rule per cell
    const int r = tid & (CFAR_TH - 1), cb = (tid / CFAR_TH) * GM_SEG;
    const int gi = r0 + r;
    const int lr = r + HA;
    double so = 0.0, sg = 0.0;
    for (int d = -a.orr; d <= a.orr; ++d) so += vo[r][HR + cb + d];
    for (int d = -a.gr; d <= a.gr; ++d) sg += vg[r][HR + cb + d];
    unsigned det = 0;
    double pw[GM_SEG], mn[GM_SEG];
#pragma unroll
    for (int q = 0; q < GM_SEG; ++q) {
        const int lc = HR + cb + q;
        if (q > 0) {
            so += vo[r][lc + a.orr]; so -= vo[r][lc - 1 - a.orr];
            sg += vg[r][lc + a.gr]; sg -= vg[r][lc - 1 - a.gr];
        }
        const int gj = c0 + cb + q;
        const int n_train = train_count(gi, gj, a.ga, a.gr, a.oa, a.orr, a.n_az, a.n_rg);
        const float mc = tile[lr][lc];
        const double p = (double)mc * (double)mc;
        const double mean = fmax(so - sg, 0.0) / (double)max(n_train, 1);
        pw[q] = p;
        mn[q] = mean;
        const bool hit = gi < a.n_az && gj < a.n_rg && n_train >= a.min_train && p > 0.0 && p > a.alpha * mean &&
                         guard_box_peak<LW>(tile, lr, lc, mc, a.ga, a.gr);
        det |= (unsigned)hit << q;
    }

    // compaction: the wave's reports get consecutive slots from one atomic
    const int lane = tid & 63;
    unsigned off[GM_SEG];
    unsigned total = 0;
#pragma unroll
    for (int q = 0; q < GM_SEG; ++q) {
        unsigned hits;
        off[q] = total + lane_rank((det >> q) & 1u, hits);
        total += hits;
    }
    if (total == 0) return;                                       // wave-uniform
    unsigned base = 0;
    if (lane == 0) {
        base = atomicAdd(&a.hdr->count, total);
        if (base + total > (unsigned)a.max_det) atomicOr(&a.hdr->overflow, 1u);
    }
    base = __shfl(base, 0);
#pragma unroll
    for (int q = 0; q < GM_SEG; ++q) {
        const unsigned slot = base + off[q];
        if (((det >> q) & 1u) && slot < (unsigned)a.max_det) store_bare_report(a.rep + slot, gi, c0 + cb + q, pw[q], mn[q]);
    }
}

hipError_t launch_gmti_cfar(const GmtiCfarArgs& a, hipStream_t st) {
    return launch_cfar_tiles(a.hdr, a.n_az, a.n_rg, a.oa, a.orr, st, [&](auto ha, auto hr, dim3 grid) {
        hipLaunchKernelGGL((gmti_cfar_kernel<ha(), hr()>), grid, dim3(CFAR_THREADS), 0, st, a);
    });
}

// Refine: one thread per report.  Its rank in (i, j) order is the number of smaller keys in the list (keys staged through LDS,
// 256 at a time), so the sorted list does not depend on the order in which the CFAR waves appended.  The interferogram is summed
// in fp64 over the 3 x 3 neighbourhood clipped to the image.
__global__ __launch_bounds__(REFINE_THREADS) void gmti_refine_kernel(const float2* __restrict__ s1, const float2* __restrict__ s2, int n_az,
                                                                int n_rg, double cc, double cs, const sarx_gmti_report* __restrict__ src,
                                                                sarx_gmti_report* __restrict__ dst, const sarx_gmti_header* hdr,
                                                                int max_det) {
    __shared__ long long keys[REFINE_THREADS];
    const int n = (int)min(hdr->count, (unsigned)max_det);
    if ((int)(blockIdx.x * REFINE_THREADS) >= n) return;              // workgroup-uniform
    const int t = blockIdx.x * REFINE_THREADS + threadIdx.x;
    sarx_gmti_report rep{};
    long long mine = LLONG_MAX;
    if (t < n) {
        rep = src[t];
        mine = (long long)rep.i * n_rg + rep.j;
    }
    int rank = 0;
    for (int b = 0; b < n; b += REFINE_THREADS) {
        __syncthreads();
        const int k = b + threadIdx.x;
        keys[threadIdx.x] = k < n ? (long long)src[k].i * n_rg + src[k].j : LLONG_MAX;
        __syncthreads();
        const int lim = min(REFINE_THREADS, n - b);
        for (int q = 0; q < lim; ++q) rank += keys[q] < mine;
    }
    if (t >= n) return;
    double ire = 0.0, iim = 0.0;
    for (int di = -1; di <= 1; ++di) {
        const int i = rep.i + di;
        if (i < 0 || i >= n_az) continue;
        for (int dj = -1; dj <= 1; ++dj) {
            const int j = rep.j + dj;
            if (j < 0 || j >= n_rg) continue;
            const size_t idx = (size_t)i * n_rg + j;
            const float2 a = s1[idx], b = s2[idx];
            const double br = b.x * cc - b.y * cs, bi = b.x * cs + b.y * cc;     // slc2 e^{j cal}
            ire += a.x * br + a.y * bi;                                          // slc1 conj(.)
            iim += a.y * br - a.x * bi;
        }
    }
    const size_t c = (size_t)rep.i * n_rg + rep.j;
    const float2 a = s1[c], b = s2[c];
    rep.interf_re = ire;
    rep.interf_im = iim;
    rep.mag1 = hypotf(a.x, a.y);
    rep.mag2 = hypotf(b.x, b.y);
    dst[rank] = rep;
}

hipError_t launch_gmti_refine(const float2* s1, const float2* s2, int n_az, int n_rg, double cal_phase, const sarx_gmti_report* src,
                              sarx_gmti_report* dst, const sarx_gmti_header* hdr, int max_det, hipStream_t st) {
    const int blocks = (max_det + REFINE_THREADS - 1) / REFINE_THREADS;
    hipLaunchKernelGGL(gmti_refine_kernel, dim3(blocks), dim3(REFINE_THREADS), 0, st, s1, s2, n_az, n_rg, cos(cal_phase), sin(cal_phase),
                       src, dst, hdr, max_det);
    return hipGetLastError();
}

}  // namespace sarx
