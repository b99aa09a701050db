// Sliding-window coherence (include/sarx_coherence.h): S12 = sum a conj(b), S11 = sum |a|^2, S22 = sum |b|^2 over a clipped box
// around every pixel, g = S12 / sqrt(S11 S22), the change rule and its summary.
//
// One workgroup of 256 threads per tile of COH_TH x COH_TW output pixels.  The box sums are separable and fp64 throughout.
//
// Azimuth direction, in registers: thread t owns image column c0 - hr + t (the tile's columns and a halo of exactly hr on each
// side; the threads past COH_TW + 2 hr carry zeros) and walks down the tile.  Its four running sums start as the direct sum of the
// window of row r0 - 1 and slide one row at a time: the row that leaves is subtracted first, then the row that enters is added,
// both from fp64 products formed on the spot (the leaving row is loaded again: it was read 2 ha + 1 rows ago by the same thread and
// comes from cache).  With ha = 0 nothing slides: the sums are set to the row's own products.  Rows are taken four at a time: the
// sixteen loads of a group are issued before the first is used, every address is clamped into the image and the value outside it
// is replaced by zero afterwards, so no load sits in a predicated block.
//
// Range direction, through LDS: after COH_R rows the column sums lie in LDS (4 x COH_R x 256 doubles, one plane per quantity,
// so neighbouring lanes write neighbouring doubles).  Thread (row = t / 32, segment = t % 32) then forms the sums of COH_SEG = 7
// neighbouring output pixels of that row: a direct sum over the 2 hr + 1 column sums of the first, then one subtraction and one
// addition per quantity and pixel.  7 is odd: the 32 lanes of a half-wave read doubles 14 dwords apart, which fall on 32 different
// bank pairs.  LDS traffic per pixel: 32 B written, (2 hr + 1 + 12) / 7 x 32 B read (60 B at hr = 0 .. 206 B at hr = 16).
//
// A running sum that has held a large power keeps a residue of it (2^-53 of that power per addition) after the power has left the
// window.  That bounds the error relative to a sum of comparable size, but not relative to a sum that should be exactly zero, so a
// fifth quantity runs beside the four: the number of cells of the window whose sample is non-zero, per image, in integers.  Where
// it is zero the sum is zero and g = 0 as the header says.
//
// Summary: every thread keeps its counts and its fp64 sum of the emitted coh in pixel order, the workgroup reduces them (shuffles
// per wave, waves in order) into one CohPartial of the workspace, and a second launch of one workgroup adds the partials in a fixed
// order.  No atomics.
#include "coherence.h"

#include "gmti_dev.hpp"

namespace sarx {

typedef float2 cf;

static constexpr int COH_THREADS = 256;
static constexpr int COH_R = 8;                // rows per pass through LDS
static constexpr int COH_SEG = 7;              // output pixels per thread and pass
static constexpr int COH_G = 4;                // rows per group of loads
static constexpr int COH_F_THREADS = 1024;
static_assert(COH_TW == 32 * COH_SEG && COH_TW + 2 * SARX_COH_MAX_HALF <= COH_THREADS, "a tile row and its halo fit the workgroup");
static_assert(COH_TH % COH_R == 0 && COH_R % COH_G == 0 && COH_R * 32 == COH_THREADS, "passes and groups are whole");

struct CohSums {
    double r, i, s11, s22;
    unsigned n;                                // cells with a non-zero sample: a's in the low half, b's in the high half
};

// adds (SUB: subtracts) the products of one cell; every product is exact in fp64
template <bool SUB> __device__ __forceinline__ void coh_cell(cf a, cf b, bool ok, CohSums& s) {
    const double ax = ok ? (double)a.x : 0.0, ay = ok ? (double)a.y : 0.0;
    const double bx = ok ? (double)b.x : 0.0, by = ok ? (double)b.y : 0.0;
    const double pax = SUB ? -ax : ax, pay = SUB ? -ay : ay, pbx = SUB ? -bx : bx, pby = SUB ? -by : by;
    s.r = fma(pax, bx, s.r); s.r = fma(pay, by, s.r);                     // a conj(b)
    s.i = fma(pay, bx, s.i); s.i = fma(-pax, by, s.i);
    s.s11 = fma(pax, ax, s.s11); s.s11 = fma(pay, ay, s.s11);
    s.s22 = fma(pbx, bx, s.s22); s.s22 = fma(pby, by, s.s22);
    const unsigned nz = ((ax != 0.0 || ay != 0.0) ? 1u : 0u) + ((bx != 0.0 || by != 0.0) ? 0x10000u : 0u);
    s.n = SUB ? s.n - nz : s.n + nz;
}

template <bool IG, bool CH> __global__ __launch_bounds__(COH_THREADS) void coherence_kernel(CoherenceArgs p) {
    __shared__ double V[4][COH_R][COH_THREADS];
    __shared__ unsigned VN[COH_R][COH_THREADS];
    __shared__ CohPartial red[COH_THREADS / 64];
    const int tid = threadIdx.x;
    const int ha = p.ha, hr = p.hr, n_az = p.n_az, n_rg = p.n_rg;
    const int c0 = blockIdx.x * COH_TW, r0 = blockIdx.y * COH_TH;
    const int gc = c0 - hr + tid;
    const bool col_in = gc >= 0 && gc < n_rg && tid < COH_TW + 2 * hr;
    const size_t cc = (size_t)min(max(gc, 0), n_rg - 1);
    const cf* pa = p.a + cc;
    const cf* pb = p.b + cc;

    // the window of row r0 - 1, summed directly
    CohSums s{0.0, 0.0, 0.0, 0.0, 0u};
    for (int i = r0 - 1 - ha; i <= r0 - 1 + ha; i += COH_G) {
        cf A[COH_G], B[COH_G];
#pragma unroll
        for (int u = 0; u < COH_G; ++u) {
            const size_t off = (size_t)min(max(i + u, 0), n_az - 1) * n_rg;
            A[u] = pa[off];
            B[u] = pb[off];
        }
#pragma unroll
        for (int u = 0; u < COH_G; ++u) {
            const int row = i + u;
            coh_cell<false>(A[u], B[u], col_in && row >= 0 && row < n_az && row <= r0 - 1 + ha, s);
        }
    }

    const int hrow = tid >> 5, seg = tid & 31;       // the range direction's work of this thread
    const int lc0 = hr + seg * COH_SEG;              // LDS column of its first output pixel
    unsigned long long n_tested = 0, n_changed = 0;
    double sum_coh = 0.0;

    for (int rb = r0; rb < r0 + COH_TH && rb < n_az; rb += COH_R) {
#pragma unroll
        for (int h = 0; h < COH_R; h += COH_G) {
            cf EA[COH_G], EB[COH_G], LA[COH_G], LB[COH_G];
#pragma unroll
            for (int u = 0; u < COH_G; ++u) {
                const int i = rb + h + u;
                const int re = i + ha, rl = ha ? i - 1 - ha : re;         // ha = 0: nothing leaves; the same line again, not used
                const size_t oe = (size_t)min(re, n_az - 1) * n_rg, ol = (size_t)min(max(rl, 0), n_az - 1) * n_rg;
                EA[u] = pa[oe];
                EB[u] = pb[oe];
                LA[u] = pa[ol];
                LB[u] = pb[ol];
            }
#pragma unroll
            for (int u = 0; u < COH_G; ++u) {
                const int i = rb + h + u;
                const int re = i + ha, rl = i - 1 - ha;
                if (ha == 0) s = CohSums{0.0, 0.0, 0.0, 0.0, 0u};
                else coh_cell<true>(LA[u], LB[u], col_in && rl >= 0 && rl < n_az, s);
                coh_cell<false>(EA[u], EB[u], col_in && re < n_az, s);
                V[0][h + u][tid] = s.r;
                V[1][h + u][tid] = s.i;
                V[2][h + u][tid] = s.s11;
                V[3][h + u][tid] = s.s22;
                VN[h + u][tid] = s.n;
            }
        }
        __syncthreads();

        const int gi = rb + hrow;
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        unsigned tn = 0;
        for (int d = -hr; d <= hr; ++d) {
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] += V[q][hrow][lc0 + d];
            tn += VN[hrow][lc0 + d];
        }
        const int rows_n = box_extent(min(gi, n_az - 1), ha, n_az);
#pragma unroll
        for (int k = 0; k < COH_SEG; ++k) {
            const int lc = lc0 + k;
            const int gj = c0 + seg * COH_SEG + k;
            if (k > 0) {
                if (hr == 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) t[q] = V[q][hrow][lc];
                    tn = VN[hrow][lc];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { t[q] -= V[q][hrow][lc - 1 - hr]; t[q] += V[q][hrow][lc + hr]; }
                    tn = tn - VN[hrow][lc - 1 - hr] + VN[hrow][lc + hr];
                }
            }
            const double s11 = (tn & 0xffffu) ? t[2] : 0.0, s22 = (tn >> 16) ? t[3] : 0.0;
            const double den = s11 * s22;
            const double inv = den > 0.0 ? rsqrt(den) : 0.0;
            const double g_re = t[0] * inv, g_im = t[1] * inv;
            const float coh = fminf((float)sqrt(g_re * g_re + g_im * g_im), 1.f);
            const bool inside = gi < n_az && gj < n_rg;
            if (inside) {
                const size_t idx = (size_t)gi * n_rg + gj;
                p.coh[idx] = coh;
                if (IG) p.igram[idx] = make_float2((float)g_re, (float)g_im);
                if (CH) {
                    const double need = p.power_floor * (double)(rows_n * box_extent(gj, hr, n_rg));
                    const bool tested = s11 >= need && s22 >= need;
                    const bool changed = tested && coh < p.threshold;
                    if (p.mask) p.mask[idx] = changed ? 2 : (tested ? 1 : 0);
                    n_tested += tested ? 1u : 0u;
                    n_changed += changed ? 1u : 0u;
                    sum_coh += tested ? (double)coh : 0.0;
                }
            }
        }
        __syncthreads();                              // the next pass overwrites the column sums
    }

    if (CH && p.part) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            n_tested += __shfl_down(n_tested, off);
            n_changed += __shfl_down(n_changed, off);
            sum_coh += __shfl_down(sum_coh, off);
        }
        if ((tid & 63) == 0) red[tid >> 6] = CohPartial{n_tested, n_changed, sum_coh};
        __syncthreads();
        if (tid == 0) {
            CohPartial w = red[0];
#pragma unroll
            for (int k = 1; k < COH_THREADS / 64; ++k) { w.n_tested += red[k].n_tested; w.n_changed += red[k].n_changed; w.sum_coh += red[k].sum_coh; }
            p.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = w;
        }
    }
}

// the workgroups' partials in a fixed order: per thread in rising tile index, waves by shuffles, waves in order
__global__ __launch_bounds__(COH_F_THREADS) void coherence_finish_kernel(const CohPartial* __restrict__ part, unsigned tiles, int n_az,
                                                                          int n_rg, sarx_coherence_summary* out) {
    constexpr int WAVES = COH_F_THREADS / 64;
    __shared__ CohPartial red[WAVES];
    const int tid = threadIdx.x;
    unsigned long long n_tested = 0, n_changed = 0;
    double sum_coh = 0.0;
    for (unsigned k = tid; k < tiles; k += COH_F_THREADS) {
        n_tested += part[k].n_tested;
        n_changed += part[k].n_changed;
        sum_coh += part[k].sum_coh;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_tested += __shfl_down(n_tested, off);
        n_changed += __shfl_down(n_changed, off);
        sum_coh += __shfl_down(sum_coh, off);
    }
    if ((tid & 63) == 0) red[tid >> 6] = CohPartial{n_tested, n_changed, sum_coh};
    __syncthreads();
    if (tid == 0) {
        CohPartial w = red[0];
        for (int k = 1; k < WAVES; ++k) { w.n_tested += red[k].n_tested; w.n_changed += red[k].n_changed; w.sum_coh += red[k].sum_coh; }
        sarx_coherence_summary sm;
        sm.n_tested = w.n_tested; sm.n_changed = w.n_changed; sm.sum_coh = w.sum_coh;
        sm.n_az = (uint32_t)n_az; sm.n_rg = (uint32_t)n_rg;
        for (int k = 0; k < 8; ++k) sm.reserved[k] = 0u;
        *out = sm;
    }
}

hipError_t launch_coherence(const CoherenceArgs& a, hipStream_t st) {
    const dim3 grid(coherence_tiles_rg(a.n_rg), coherence_tiles_az(a.n_az));
    const bool change = a.mask || a.summary;
    if (a.igram) {
        if (change) hipLaunchKernelGGL((coherence_kernel<true, true>), grid, dim3(COH_THREADS), 0, st, a);
        else hipLaunchKernelGGL((coherence_kernel<true, false>), grid, dim3(COH_THREADS), 0, st, a);
    } else {
        if (change) hipLaunchKernelGGL((coherence_kernel<false, true>), grid, dim3(COH_THREADS), 0, st, a);
        else hipLaunchKernelGGL((coherence_kernel<false, false>), grid, dim3(COH_THREADS), 0, st, a);
    }
    if (a.summary)
        hipLaunchKernelGGL(coherence_finish_kernel, dim3(1), dim3(COH_F_THREADS), 0, st, a.part, grid.x * grid.y, a.n_az, a.n_rg, a.summary);
    return hipGetLastError();
}

}  // namespace sarx
