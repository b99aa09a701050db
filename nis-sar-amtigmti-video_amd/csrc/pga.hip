// Phase-gradient autofocus (include/sarx_pga.h): the estimate launch, the integrate launch and the apply launch.
//
// Estimate launch: grid = tiles x frames.  A workgroup holds WT = 4096 / L columns of one frame as the [L rows x WT cols] Stockham
// tile of fft_core.hpp, 16 points per thread, 256 threads for every L.  The first read takes each column's peak row, power sum and
// the tile's s2, s4 through fixed trees in LDS.  The second read (the tile is in cache) loads through the rotated and windowed index
// straight into the transform's input order: rows outside the window and columns that are not used are never loaded.  After
// stockham_run the spectrum goes through LDS once, in fftshift order and with one pad element per row, so that a thread per bin adds
// |G[k]|^2 and G[k] conj(G[k-1]) over the tile's columns in column order, in fp64.  The tile's row of partial sums goes to the
// workspace.  Integrate launch: one workgroup per frame adds the rows in tile order (the three scalars per tile as a strided sum
// and a tree), takes the arguments, scans, detrends, updates phi_tot and writes the record.  Apply launch: load tile, forward, multiply by cis of the fp64 phase reduced to revolutions,
// inverse in the reversed plan order (which starts from the forward transform's registers), store.  No atomics anywhere.
#include "pga.h"
#include "fft_core.hpp"

#include <climits>

namespace sarx {

template <int L> struct PgaCfg {
    static constexpr int WT = pga_tile_cols(L);
    static constexpr int T = Plan<L>::T;           // threads per column (16 points each)
    static constexpr int THREADS = T * WT;
    static constexpr int LDS = (WT + 1) * L;       // cf elements: the exchange image [L x WT]; the spectrum image [L x (WT + 1)]
    static_assert(Plan<L>::P == 16 && THREADS == 256, "16 points per thread, 256 threads");
    static_assert(LdsSize<L, WT>::value <= LDS && LDS >= 4 * THREADS, "LDS reuse");
    static_assert(Edge<L, false>::R_last == Edge<L, true>::R_first, "the inverse starts from the forward transform's registers");
};

// Sum of x over the tile, as a fixed tree in red[256]: first over the T threads of each column (the column's sum comes back in
// col), then over the WT columns.  The total is red[0] once the function returns.
template <int T, int WT> __device__ __forceinline__ double tile_sum(double x, double* red, int t, double& col) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
#pragma unroll
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s) red[tid] += red[tid + s * WT];
        __syncthreads();
    }
    col = red[tid % WT];
    __syncthreads();
#pragma unroll
    for (int s = WT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

template <int L> __global__ __launch_bounds__(256) void pga_estimate_kernel(PgaEstimateArgs a) {
    using CFG = PgaCfg<L>;
    using E = Edge<L, false>;
    constexpr int WT = CFG::WT, T = CFG::T, R0 = E::R_first, RL = E::R_last, LD = WT + 1;
    __shared__ __attribute__((aligned(16))) cf lds[CFG::LDS];
    double* red = reinterpret_cast<double*>(lds);                  // [256]
    float* rp = reinterpret_cast<float*>(lds + 256);               // [256]
    int* ri = reinterpret_cast<int*>(lds + 384);                   // [256]
    int* flag = reinterpret_cast<int*>(lds + 512);                 // [WT]
    const int tid = threadIdx.x, c = tid % WT, t = tid / WT;
    const int tile = blockIdx.x, f = blockIdx.y;
    const int col = tile * WT + c;
    const bool valid = col < a.g.n_rg;
    const size_t ld = a.g.ld;
    const float2* img = a.src + (size_t)f * a.g.frame_stride + (size_t)min(col, a.g.n_rg - 1);

    // first read: rows t, t + T, ...; per thread the peak (ties: the smaller row), the power sum and the sum of squared powers
    cf x[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) x[q] = img[(size_t)(t + q * T) * ld];
    float bp = -1.f;
    int bi = INT_MAX;
    double e2 = 0.0, e4 = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float p = valid ? fmaf(x[q].x, x[q].x, x[q].y * x[q].y) : 0.f;
        e2 += (double)p;
        e4 += (double)(p * p);
        if (p > bp) { bp = p; bi = t + q * T; }
    }
    double col_e2, col_e4;
    const double s2 = tile_sum<T, WT>(e2, red, t, col_e2);
    const double s4 = tile_sum<T, WT>(e4, red, t, col_e4);
    __syncthreads();
    rp[tid] = bp;
    ri[tid] = bi;
    __syncthreads();
#pragma unroll
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s) {
            const float po = rp[tid + s * WT];
            const int io = ri[tid + s * WT];
            if (po > rp[tid] || (po == rp[tid] && io < ri[tid])) { rp[tid] = po; ri[tid] = io; }
        }
        __syncthreads();
    }
    const float pk = rp[c];
    const bool used = valid && pk > 0.f && (double)pk * (double)L >= a.min_contrast * col_e2;     // c_j = pk / (col_e2 / L)
    const int rj = used ? ri[c] : 0;
    if (t == 0) flag[c] = used ? 1 : 0;
    __syncthreads();
    double* row = a.work + ((size_t)f * gridDim.x + tile) * pga_row_doubles(L);
    if (tid == 0) {
        int n = 0;
        for (int cc = 0; cc < WT; ++cc) n += flag[cc];
        row[3 * L + 0] = s2;
        row[3 * L + 1] = s4;
        row[3 * L + 2] = (double)n;
        row[3 * L + 3] = 0.0;
    }

    // second read: point n of the rotated, windowed column is row (n + r_j) mod L when min(n, L - n) <= h, else 0
    cf v[16];
#pragma unroll
    for (int b = 0; b < 16 / R0; ++b)
#pragma unroll
        for (int r = 0; r < R0; ++r) {
            const int n = E::in_index(t, b, r);
            const bool in = used && min(n, L - n) <= a.half_width;
            v[b * R0 + r] = in ? img[(size_t)((n + rj) & (L - 1)) * ld] : make_float2(0.f, 0.f);
        }
    __syncthreads();                                               // flag read before the exchange image is written
    stockham_run<L, WT, false, false, 0, false, true>(v, t, c, lds, nullptr);
    __syncthreads();                                               // the last gather is done
#pragma unroll
    for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
        for (int r = 0; r < RL; ++r) lds[((E::out_index(t, b, r) + L / 2) & (L - 1)) * LD + c] = v[b * RL + r];
    __syncthreads();
    for (int k = tid; k < L; k += CFG::THREADS) {
        double P = 0.0, sr = 0.0, si = 0.0;
        const cf* g1 = lds + k * LD;
        const cf* g0 = lds + (k > 0 ? k - 1 : 0) * LD;
        for (int cc = 0; cc < WT; ++cc) {
            const double gx = g1[cc].x, gy = g1[cc].y, hx = g0[cc].x, hy = g0[cc].y;
            P += gx * gx + gy * gy;
            sr += gx * hx + gy * hy;                               // G[k] conj(G[k-1])
            si += gy * hx - gx * hy;
        }
        row[k] = P;
        row[L + k] = k > 0 ? sr : 0.0;
        row[2 * L + k] = k > 0 ? si : 0.0;
    }
}

// N values per thread summed over the 256 threads as one fixed tree; the sums come back in x for every thread
template <int N> __device__ __forceinline__ void block_sums(double (&x)[N], double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) red[i * 256 + tid] = x[i];
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int i = 0; i < N; ++i) red[i * 256 + tid] += red[i * 256 + tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = red[i * 256];
}

template <int L> __global__ __launch_bounds__(256) void pga_integrate_kernel(PgaEstimateArgs a, int tiles) {
    constexpr int NB = L >= 256 ? L / 256 : 1;                     // bins per thread: k = tid + m 256
    __shared__ double red[5 * 256];
    __shared__ double scan[2][L];
    __shared__ int sup[L];
    const int tid = threadIdx.x, f = blockIdx.x;
    const size_t stride = pga_row_doubles(L);
    const double* rows = a.work + (size_t)f * tiles * stride;

    double P[NB], sr[NB], si[NB];
    double pmax = 0.0;
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        const int k = tid + m * 256;
        P[m] = sr[m] = si[m] = 0.0;
        if (k < L)
#pragma unroll 8
            for (int tl = 0; tl < tiles; ++tl) {                   // tile order; unrolled so that eight tiles' loads are in flight
                const double* r = rows + (size_t)tl * stride;
                P[m] += r[k];
                sr[m] += r[L + k];
                si[m] += r[2 * L + k];
            }
        pmax = fmax(pmax, P[m]);
    }
    __syncthreads();
    red[tid] = pmax;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double thr = a.power_floor * red[0];
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        const int k = tid + m * 256;
        if (k < L) sup[k] = P[m] > thr ? 1 : 0;
    }
    __syncthreads();
    bool s_k[NB];
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        const int k = tid + m * 256;
        s_k[m] = k < L && sup[k];
        if (k < L) scan[0][k] = (k >= 1 && sup[k] && sup[k - 1]) ? atan2(si[m], sr[m]) : 0.0;
    }
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int off = 1; off < L; off <<= 1) {                        // inclusive scan, the same tree for every frame
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            const int k = tid + m * 256;
            if (k < L) scan[cur ^ 1][k] = k >= off ? scan[cur][k] + scan[cur][k - off] : scan[cur][k];
        }
        __syncthreads();
        cur ^= 1;
    }
    // least-squares line over the supported bins, x = k - L / 2
    double phi[NB];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        const int k = tid + m * 256;
        phi[m] = k < L ? scan[cur][k] : 0.0;
        if (s_k[m]) {
            const double xk = (double)(k - L / 2);
            acc[0] += 1.0;
            acc[1] += xk;
            acc[2] += xk * xk;
            acc[3] += phi[m];
            acc[4] += xk * phi[m];
        }
    }
    block_sums<5>(acc, red);
    const double n = acc[0];
    double slope = 0.0, icpt = 0.0;
    if (n >= 2.0) {
        slope = (n * acc[4] - acc[1] * acc[3]) / (n * acc[2] - acc[1] * acc[1]);
        icpt = (acc[3] - slope * acc[1]) / n;
    }
    double sq[1] = {0.0};
#pragma unroll
    for (int m = 0; m < NB; ++m) {
        const int k = tid + m * 256;
        phi[m] = (s_k[m] && n >= 2.0) ? phi[m] - (icpt + slope * (double)(k - L / 2)) : 0.0;
        sq[0] += phi[m] * phi[m];
    }
    block_sums<1>(sq, red);
    if (a.update) {
        double* ph = a.phase + (size_t)f * L;
#pragma unroll
        for (int m = 0; m < NB; ++m) {
            const int k = tid + m * 256;
            if (k < L) ph[k] = a.first ? phi[m] : ph[k] + phi[m];
        }
    }
    double tot[3] = {0.0, 0.0, 0.0};                             // s2, s4, used columns: thread t takes tiles t, t + 256, ..., then the tree
    for (int tl = tid; tl < tiles; tl += 256) {
        const double* r = rows + (size_t)tl * stride + 3 * L;
        tot[0] += r[0];
        tot[1] += r[1];
        tot[2] += r[2];
    }
    block_sums<3>(tot, red);
    if (tid == 0) {
        sarx_pga_record o;
        o.s2 = tot[0];
        o.s4 = tot[1];
        o.rms_phase = n >= 2.0 ? sqrt(sq[0] / n) : 0.0;
        o.n_cols_used = (int)tot[2];
        o.n_bins_supported = (int)n;
        a.rec[(size_t)f * a.rec_stride] = o;
    }
}

template <int L> __global__ __launch_bounds__(256) void pga_apply_kernel(PgaApplyArgs a) {
    using CFG = PgaCfg<L>;
    using EF = Edge<L, false>;
    using EI = Edge<L, true>;
    constexpr int WT = CFG::WT, R0 = EF::R_first, RM = EF::R_last, RL = EI::R_last;
    __shared__ __attribute__((aligned(16))) cf lds[LdsSize<L, WT>::value];
    const int tid = threadIdx.x, c = tid % WT, t = tid / WT;
    const int f = blockIdx.y;
    const int col = blockIdx.x * WT + c;
    const bool valid = col < a.g.n_rg;
    const size_t ld = a.g.ld;
    const size_t origin = (size_t)f * a.g.frame_stride + (size_t)min(col, a.g.n_rg - 1);
    const float2* img = a.src + origin;
    const double* ph = a.phase + (size_t)f * a.phase_stride;
    cf v[16];
#pragma unroll
    for (int b = 0; b < 16 / R0; ++b)
#pragma unroll
        for (int r = 0; r < R0; ++r) v[b * R0 + r] = img[(size_t)EF::in_index(t, b, r) * ld];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = valid ? v[q] : make_float2(0.f, 0.f);
    stockham_run<L, WT, false, false, 0, false, true>(v, t, c, lds, nullptr);
    const float inv_l = 1.0f / (float)L;
#pragma unroll
    for (int b = 0; b < 16 / RM; ++b)
#pragma unroll
        for (int r = 0; r < RM; ++r) {
            const int k = (EF::out_index(t, b, r) + L / 2) & (L - 1);
            const cf y = cmul(v[b * RM + r], cis_rev(a.sign_rev * ph[k]));
            v[b * RM + r] = make_float2(y.x * inv_l, y.y * inv_l);
        }
    __syncthreads();                                               // the forward transform's last gather is done
    stockham_run<L, WT, true, true, 0, false, true>(v, t, c, lds, nullptr);
    if (valid) {
        float2* out = a.dst + origin;
#pragma unroll
        for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
            for (int q = 0; q < RL; ++q) out[(size_t)EI::out_index(t, b, q) * ld] = v[b * RL + q];
    }
}

template <int L> static void estimate_l(const PgaEstimateArgs& a, hipStream_t st) {
    const int tiles = pga_tiles(L, a.g.n_rg);
    hipLaunchKernelGGL((pga_estimate_kernel<L>), dim3(tiles, a.g.n_frames), dim3(256), 0, st, a);
    hipLaunchKernelGGL((pga_integrate_kernel<L>), dim3(a.g.n_frames), dim3(256), 0, st, a, tiles);
}
template <int L> static void apply_l(const PgaApplyArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((pga_apply_kernel<L>), dim3(pga_tiles(L, a.g.n_rg), a.g.n_frames), dim3(256), 0, st, a);
}

hipError_t launch_pga_estimate(const PgaEstimateArgs& a, hipStream_t st) {
    switch (a.g.L) {
        case 64: estimate_l<64>(a, st); break;
        case 128: estimate_l<128>(a, st); break;
        case 256: estimate_l<256>(a, st); break;
        case 512: estimate_l<512>(a, st); break;
        case 1024: estimate_l<1024>(a, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_pga_apply(const PgaApplyArgs& a, hipStream_t st) {
    switch (a.g.L) {
        case 64: apply_l<64>(a, st); break;
        case 128: apply_l<128>(a, st); break;
        case 256: apply_l<256>(a, st); break;
        case 512: apply_l<512>(a, st); break;
        case 1024: apply_l<1024>(a, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sarx
