// GMTI refocus (include/sarx_refocus.h): per report, an L x W chip of the DPCA difference (or of slc1) is re-compressed in
// azimuth for n_hyp platform-speed hypotheses and each result is scored by its sharpness sum |Y|^4 / (sum |x|^2)^2.
//
// Curve launch: grid = reports x hypothesis groups of RF_HG.  A workgroup holds the chip as RF_WT >= W columns of the
// [L rows x WT cols] Stockham tile of fft_core.hpp (columns W .. WT-1 and columns outside the image are zero), all of its loads
// issued before the first wait.  The forward transform runs once (plan order REV = false), the spectrum stays in registers, and
// per hypothesis the phase is applied in place and the inverse runs in plan order REV = true, whose first stage reads exactly
// the registers the forward transform's last stage left.  The phase rate g_k(f) = 2 (D(f; V'_k) - D(f; V_r)) / lambda is
// evaluated once per frequency bin in fp64 into LDS, scaled by each column's range in fp64, reduced to revolutions and turned
// into an fp32 cis (cis_rev).  Record launch: one workgroup per report takes the argmax of its curve, recomputes Y_{k*}, and
// writes the peak, the record and the optional chip.  Every reduction is a fixed tree in LDS: no atomics, deterministic.
#include "refocus.h"
#include "fft_core.hpp"

#include <climits>

namespace sarx {

static constexpr int RF_HG = 8;                    // hypotheses per workgroup of the curve launch

template <int L, int WT> struct RfCfg {
    static constexpr int T = Plan<L>::T;           // threads per column (16 points each)
    static constexpr int THREADS = T * WT;
    static constexpr int LDS = LdsSize<L, WT>::value;   // cf elements: the exchange image, reused for g_k(f) and the reductions
    static_assert(Plan<L>::P == 16, "16 points per thread");
    static_assert(Edge<L, false>::R_last == Edge<L, true>::R_first, "the inverse starts from the forward transform's registers");
    static_assert(LDS >= L && LDS >= 2 * THREADS, "LDS reuse");
};

// sum over the workgroup in a fixed order (every LDS phase of these kernels starts with a barrier)
template <int N> __device__ __forceinline__ double block_sum(double x, double* red) {
    __syncthreads();
    red[threadIdx.x] = x;
    __syncthreads();
#pragma unroll
    for (int s = 512; s > 0; s >>= 1) {
        if (s < N) {
            if ((int)threadIdx.x < s && (int)threadIdx.x + s < N) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
    }
    return red[0];
}
template <int N> __device__ __forceinline__ float block_max(float x, float* red) {
    __syncthreads();
    red[threadIdx.x] = x;
    __syncthreads();
#pragma unroll
    for (int s = 512; s > 0; s >>= 1) {
        if (s < N) {
            if ((int)threadIdx.x < s && (int)threadIdx.x + s < N) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
            __syncthreads();
        }
    }
    return red[0];
}

// first chip row of report r; false when the workgroup has nothing to do (overflowed slot, or r past the list)
__device__ __forceinline__ bool chip_origin(const RefocusArgs& a, int r, int& i0, int& j) {
    const sarx_gmti_header h = *a.hdr;
    if (h.overflow || r >= (int)min(h.count, (unsigned)a.max_det) || a.L > a.n_az) return false;
    const int i = a.rep[r].i;
    j = a.rep[r].j;
    i0 = min(max(i - a.L / 2, 0), a.n_az - a.L);
    return true;
}

// x at the first stage's input points of thread (t, c): all 32 loads are issued before any is used (addresses clamped into the
// image, values outside it zeroed afterwards)
template <int L> __device__ __forceinline__ void load_chip(const RefocusArgs& a, int i0, int col, bool valid, int t, cf* v) {
    using E = Edge<L, false>;
    constexpr int R0 = E::R_first;
    const int cc = min(max(col, 0), a.n_rg - 1);
    cf p1[16], p2[16];
#pragma unroll
    for (int b = 0; b < 16 / R0; ++b)
#pragma unroll
        for (int r = 0; r < R0; ++r) {
            const size_t idx = (size_t)(i0 + E::in_index(t, b, r)) * a.n_rg + cc;
            p1[b * R0 + r] = a.s1[idx];
            p2[b * R0 + r] = a.s2[idx];
        }
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = valid ? csub(p1[q], cmul(a.w2, p2[q])) : make_float2(0.f, 0.f);
}

// g_k(f) in revolutions per metre of range for every bin of the L-point fftfreq axis, into LDS
template <int THREADS> __device__ __forceinline__ void phase_rates(const RefocusArgs& a, double vp, double* g) {
    __syncthreads();
    for (int f = threadIdx.x; f < a.L; f += THREADS) {
        const double fr = (double)(f < a.L / 2 ? f : f - a.L) * a.prf / (double)a.L;
        const double q = 0.25 * a.lam * a.lam * fr * fr;               // (lambda f / 2)^2
        const double ar = 1.0 - q / (a.vr * a.vr), ap = 1.0 - q / (vp * vp);
        const double d = sqrt(ar < 0.0 ? 1e-9 : ar), dp = sqrt(ap < 0.0 ? 1e-9 : ap);
        const double diff = (ar < 0.0 || ap < 0.0) ? dp - d : q * (1.0 / (a.vr * a.vr) - 1.0 / (vp * vp)) / (dp + d);
        g[f] = 2.0 * diff / a.lam;
    }
    __syncthreads();
}

// spectrum X (forward transform's output order) -> Y_k (inverse's output order) in v
template <int L, int WT> __device__ __forceinline__ void refocus_one(const RefocusArgs& a, const cf* X, cf* v, double rng, double vp,
                                                                     int t, int c, cf* lds) {
    using EF = Edge<L, false>;
    constexpr int R = EF::R_last;
    const double* g = reinterpret_cast<const double*>(lds);
    phase_rates<RfCfg<L, WT>::THREADS>(a, vp, reinterpret_cast<double*>(lds));
    const float inv_l = 1.0f / (float)L;
#pragma unroll
    for (int b = 0; b < 16 / R; ++b)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const cf w = cis_rev(rng * g[EF::out_index(t, b, r)]);
            const cf y = cmul(X[b * R + r], w);
            v[b * R + r] = make_float2(y.x * inv_l, y.y * inv_l);
        }
    __syncthreads();                                               // g read before the exchange image is overwritten
    stockham_run<L, WT, true, true>(v, t, c, lds, nullptr);
}

template <int L, int WT> __global__ __launch_bounds__((RfCfg<L, WT>::THREADS)) void refocus_curve_kernel(RefocusArgs a) {
    using CFG = RfCfg<L, WT>;
    __shared__ __attribute__((aligned(16))) cf lds[CFG::LDS];
    const int r = blockIdx.x;
    int i0, j;
    if (!chip_origin(a, r, i0, j)) return;                        // workgroup-uniform
    const int c = threadIdx.x % WT, t = threadIdx.x / WT;
    const int col = j - a.W / 2 + c;
    const bool valid = c < a.W && col >= 0 && col < a.n_rg;
    cf v[16];
    load_chip<L>(a, i0, col, valid, t, v);
    double e2 = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) e2 += (double)fmaf(v[q].x, v[q].x, v[q].y * v[q].y);
    const double E = block_sum<CFG::THREADS>(e2, reinterpret_cast<double*>(lds));
    const double inv_e2 = E > 0.0 ? 1.0 / (E * E) : 0.0;
    __syncthreads();
    stockham_run<L, WT, false, false>(v, t, c, lds, nullptr);
    cf X[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) X[q] = v[q];
    const double rng = a.r0 + (double)col * a.dr;
    const int k_end = min(a.n_hyp, ((int)blockIdx.y + 1) * RF_HG);
    for (int k = blockIdx.y * RF_HG; k < k_end; ++k) {
        refocus_one<L, WT>(a, X, v, rng, a.vp[k], t, c, lds);
        double s4 = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float p = fmaf(v[q].x, v[q].x, v[q].y * v[q].y);
            s4 += (double)(p * p);
        }
        const double S = block_sum<CFG::THREADS>(s4, reinterpret_cast<double*>(lds)) * inv_e2;
        if (threadIdx.x == 0) a.curves[(size_t)r * a.n_hyp + k] = (float)S;
    }
}

template <int L, int WT> __global__ __launch_bounds__((RfCfg<L, WT>::THREADS)) void refocus_record_kernel(RefocusArgs a) {
    using CFG = RfCfg<L, WT>;
    using EI = Edge<L, true>;
    constexpr int RL = EI::R_last;
    __shared__ __attribute__((aligned(16))) cf lds[CFG::LDS];
    double* red = reinterpret_cast<double*>(lds);
    const int r = blockIdx.x;
    int i0, j;
    if (!chip_origin(a, r, i0, j)) return;                        // workgroup-uniform
    const int c = threadIdx.x % WT, t = threadIdx.x / WT;
    const int col = j - a.W / 2 + c;
    const bool valid = c < a.W && col >= 0 && col < a.n_rg;
    cf v[16];
    load_chip<L>(a, i0, col, valid, t, v);
    double e2 = 0.0, e4 = 0.0;
    float pmax = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float p = fmaf(v[q].x, v[q].x, v[q].y * v[q].y);
        e2 += (double)p;
        e4 += (double)(p * p);
        pmax = fmaxf(pmax, p);
    }
    const double E = block_sum<CFG::THREADS>(e2, red);
    const double E4 = block_sum<CFG::THREADS>(e4, red);
    const float orig = block_max<CFG::THREADS>(pmax, reinterpret_cast<float*>(lds));
    const double inv_e2 = E > 0.0 ? 1.0 / (E * E) : 0.0;

    const float* cv = a.curves + (size_t)r * a.n_hyp;
    int kb = 0;
    float sb = cv[0];
    for (int k = 1; k < a.n_hyp; ++k) {                           // ties: the smaller k
        const float s = cv[k];
        if (s > sb) { sb = s; kb = k; }
    }
    __syncthreads();
    stockham_run<L, WT, false, false>(v, t, c, lds, nullptr);
    cf X[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) X[q] = v[q];
    refocus_one<L, WT>(a, X, v, a.r0 + (double)col * a.dr, a.vp[kb], t, c, lds);

    // peak of |Y|^2 over the in-image cells: (power, linear index), larger power first, ties to the smaller index
    float bp = -1.f;
    long long bi = LLONG_MAX;
#pragma unroll
    for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
        for (int q = 0; q < RL; ++q) {
            const cf y = v[b * RL + q];
            const float p = fmaf(y.x, y.x, y.y * y.y);
            const long long li = (long long)(i0 + EI::out_index(t, b, q)) * a.n_rg + col;
            if (valid && (p > bp || (p == bp && li < bi))) { bp = p; bi = li; }
        }
    float* rp = reinterpret_cast<float*>(lds);
    long long* ri = reinterpret_cast<long long*>(lds + CFG::THREADS);
    __syncthreads();
    rp[threadIdx.x] = bp;
    ri[threadIdx.x] = bi;
    __syncthreads();
#pragma unroll
    for (int s = 512; s > 0; s >>= 1) {
        if (s < CFG::THREADS) {
            const int o = threadIdx.x + s;
            if ((int)threadIdx.x < s && o < CFG::THREADS) {
                const float po = rp[o];
                const long long io = ri[o];
                if (po > rp[threadIdx.x] || (po == rp[threadIdx.x] && io < ri[threadIdx.x])) { rp[threadIdx.x] = po; ri[threadIdx.x] = io; }
            }
            __syncthreads();
        }
    }
    if (a.chips && c < a.W) {
        float2* out = a.chips + (size_t)r * a.L * a.W;
#pragma unroll
        for (int b = 0; b < 16 / RL; ++b)
#pragma unroll
            for (int q = 0; q < RL; ++q) out[(size_t)EI::out_index(t, b, q) * a.W + c] = v[b * RL + q];
    }
    if (threadIdx.x == 0) {
        sarx_refocus_record o{};
        o.k_best = kb;
        o.i0 = i0;
        o.peak_i = (int)(ri[0] / a.n_rg);
        o.peak_j = (int)(ri[0] % a.n_rg);
        o.s_prev = kb > 0 ? cv[kb - 1] : -1.f;
        o.s_best = sb;
        o.s_next = kb + 1 < a.n_hyp ? cv[kb + 1] : -1.f;
        o.s_identity = (float)(E4 * inv_e2);
        o.peak_power = rp[0];
        o.orig_power = orig;
        a.rec[r] = o;
    }
}

template <int L, int WT> static void launch_lw(const RefocusArgs& a, hipStream_t st) {
    using CFG = RfCfg<L, WT>;
    const dim3 grid1(a.max_det, (a.n_hyp + RF_HG - 1) / RF_HG);
    hipLaunchKernelGGL((refocus_curve_kernel<L, WT>), grid1, dim3(CFG::THREADS), 0, st, a);
    hipLaunchKernelGGL((refocus_record_kernel<L, WT>), dim3(a.max_det), dim3(CFG::THREADS), 0, st, a);
}
// W is a run-time value: the tile is instantiated 1, 5 or 15 columns wide
template <int L> static void launch_l(const RefocusArgs& a, hipStream_t st) {
    if (a.W == 1) launch_lw<L, 1>(a, st);
    else if (a.W <= 5) launch_lw<L, 5>(a, st);
    else launch_lw<L, 15>(a, st);
}

hipError_t launch_refocus(const RefocusArgs& a, hipStream_t st) {
    switch (a.L) {
        case 64: launch_l<64>(a, st); break;
        case 128: launch_l<128>(a, st); break;
        case 256: launch_l<256>(a, st); break;
        case 512: launch_l<512>(a, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sarx
