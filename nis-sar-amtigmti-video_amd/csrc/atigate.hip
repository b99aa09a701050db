// GMTI ATI gate (include/sarx_atigate.h has the semantics; tests/_atigate_numpy.py restates them with math.fsum).
//
// Two launches.
//   statistics : one workgroup of 256 threads per report (blockIdx.x = report; the count comes from the device header, workgroups
//                beyond it exit).  The outer box of H x W cells (W = 2 (guard_rg + train_rg) + 1 <= 65, one more than a wave has
//                lanes) is walked as one flat index e = row W + column: thread t takes e = t, t + 256, ..., so the lanes of a wave
//                run along range inside a row and wrap into the next one, and every load is 8 bytes beside its neighbour's.  The
//                kernel is instantiated for K = 1, 2, 5, 9, 17 cells per thread (17 x 256 >= 65 x 65); every address is clamped into
//                the image and the K loads of both images are issued before the first wait (the idiom of the CFAR tile fill), the
//                contribution of a cell outside the image, outside the box or in the wrong set is dropped by a select afterwards.
//                A report reads at most 65 x 65 cells of two images, 67 KB, most of it from L2: what the launch waits for is the
//                latency of one round of loads, not HBM.
//                Sums: every product of two fp32 samples is exact in fp64 and is added on its own (no fused multiply-add), per
//                thread in rising e, then across the lanes in a butterfly (lane ^ 32, 16, ... 1: an IEEE sum does not depend on
//                the order of its two operands, so all lanes hold the same bits), then across the four waves in wave order
//                through LDS.  Thread 0 derives coh, psi, sigma and the decision and writes the record and the keep flag.
//   compaction : one workgroup of 1024 threads ranks the keep flags with gmti_dev.hpp's block_rank, 1024 reports a round, as
//                cluster.hip ranks its plots, copies the kept reports as six 8-byte words each and fills in out_index.
// No global atomics, no scratch, the same bytes in every run.
#include "atigate.h"

#include "gmti_dev.hpp"

// every fp64 operation rounds on its own: the sums are sums of exact products, thr = k_sigma * sigma is one rounded product
#pragma clang fp contract(off)

namespace sarx {

constexpr int AG_THREADS = 256;
constexpr int AG_WAVES = AG_THREADS / 64;
constexpr int AG_SUMS = 6;                          // c11, c22, c12_re, c12_im, i_re, i_im
constexpr int AGC_THREADS = 1024;
constexpr int AGC_WAVES = AGC_THREADS / 64;

template <int K> __global__ __launch_bounds__(AG_THREADS) void atigate_stats_kernel(AtiGateArgs g) {
    __shared__ double part[AG_WAVES][AG_SUMS];
    const SlotView in = slot_view(g.in, g.p.max_detections);
    if (in.unusable || blockIdx.x >= in.count) return;         // workgroup-uniform
    const int r = blockIdx.x, tid = threadIdx.x;
    const int2 ij = *reinterpret_cast<const int2*>(in.rep + r);         // i and j lead the record
    const bool valid = (unsigned)ij.x < (unsigned)g.n_az && (unsigned)ij.y < (unsigned)g.n_rg;
    const int i = valid ? ij.x : 0, j = valid ? ij.y : 0;
    const int ga = g.p.guard_az, gr = g.p.guard_rg, oa = ga + g.p.train_az, orr = gr + g.p.train_rg;
    const int la = g.p.look_az, lr = g.p.look_rg;
    const int H = 2 * oa + 1, W = 2 * orr + 1;
    const int row0 = tid / W, col0 = tid - row0 * W;
    const int drow = AG_THREADS / W, dcol = AG_THREADS - drow * W;      // what 256 cells further means in rows and columns

    // every load issued before the first wait: the address is clamped into the image, so it carries no branch
    float2 va[K], vb[K];
    {
        int row = row0, col = col0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int cr = min(max(i + row - oa, 0), g.n_az - 1), cc = min(max(j + col - orr, 0), g.n_rg - 1);
            const size_t idx = (size_t)cr * g.n_rg + cc;
            va[k] = g.a[idx];
            vb[k] = g.b[idx];
            row += drow; col += dcol;
            if (col >= W) { col -= W; ++row; }
        }
    }
    double s[AG_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    {
        int row = row0, col = col0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int di = row - oa, dj = col - orr;
            const bool inside = valid && row < H && (unsigned)(i + di) < (unsigned)g.n_az && (unsigned)(j + dj) < (unsigned)g.n_rg;
            const bool ring = inside && !(abs(di) <= ga && abs(dj) <= gr);
            const bool look = inside && abs(di) <= la && abs(dj) <= lr;          // inside the guard box: never a ring cell
            const double ar = va[k].x, ai = va[k].y, br = vb[k].x, bi = vb[k].y;
            const double t11a = ar * ar, t11b = ai * ai, t22a = br * br, t22b = bi * bi;       // exact: 24 x 24 bits
            const double trr = ar * br, tii = ai * bi, tir = ai * br, tri = ar * bi;
            s[0] += ring ? t11a : 0.0; s[0] += ring ? t11b : 0.0;
            s[1] += ring ? t22a : 0.0; s[1] += ring ? t22b : 0.0;
            s[2] += ring ? trr : 0.0;  s[2] += ring ? tii : 0.0;
            s[3] += ring ? tir : 0.0;  s[3] -= ring ? tri : 0.0;
            s[4] += look ? trr : 0.0;  s[4] += look ? tii : 0.0;
            s[5] += look ? tir : 0.0;  s[5] -= look ? tri : 0.0;
            row += drow; col += dcol;
            if (col >= W) { col -= W; ++row; }
        }
    }
#pragma unroll
    for (int q = 0; q < AG_SUMS; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_xor(s[q], off);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < AG_SUMS; ++q) part[tid >> 6][q] = s[q];
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int q = 0; q < AG_SUMS; ++q) {
        double t = part[0][q];
        for (int w = 1; w < AG_WAVES; ++w) t += part[w][q];
        s[q] = t;
    }

    sarx_atigate_stat st{};
    st.c11 = s[0]; st.c22 = s[1]; st.c12_re = s[2]; st.c12_im = s[3]; st.i_re = s[4]; st.i_im = s[5];
    if (valid) {
        st.n_train = train_count(i, j, ga, gr, oa, orr, g.n_az, g.n_rg);
        st.n_look = box_extent(i, la, g.n_az) * box_extent(j, lr, g.n_rg);
    }
    const double prod = s[0] * s[1];
    if (st.n_train < g.p.min_train) {
        st.reason = SARX_ATIGATE_REASON_TRAIN;
    } else if (prod == 0.0 || (s[4] == 0.0 && s[5] == 0.0)) {
        st.reason = SARX_ATIGATE_REASON_ZERO;
    } else {
        const double den = sqrt(prod);
        const double coh = fmin(hypot(s[2] / den, s[3] / den), 1.0);
        st.coh = coh;
        if (coh < g.p.min_coh) {
            st.reason = SARX_ATIGATE_REASON_COHERENCE;
        } else {
            const double re = s[4] * s[2] + s[5] * s[3], im = s[5] * s[2] - s[4] * s[3];
            const double c2 = coh * coh;
            st.psi = atan2(im, re);
            st.sigma = sqrt((1.0 - c2) / (2.0 * (double)st.n_look * c2));
            const double thr = g.p.k_sigma * st.sigma;
            st.status = fabs(st.psi) > thr && fabs(st.psi) >= g.p.phase_min ? SARX_ATIGATE_PASSED : SARX_ATIGATE_REJECTED;
        }
    }
    const bool kept = st.status == SARX_ATIGATE_PASSED ||
                      (st.status == SARX_ATIGATE_UNTESTED && (g.p.flags & SARX_ATIGATE_KEEP_UNTESTED) != 0);
    st.out_index = -1;                                         // the compaction launch sets the kept ones
    g.keep[r] = kept ? 1 : 0;
    if (g.stats) g.stats[r] = st;
}

__global__ __launch_bounds__(AGC_THREADS) void atigate_compact_kernel(AtiGateArgs g) {
    __shared__ int wsum[AGC_WAVES];
    const int tid = threadIdx.x;
    const SlotView in = slot_view(g.in, g.p.max_detections);
    if (in.unusable) {
        if (tid == 0) slot_close(g.out, in.count, true);
        return;
    }
    const int n = (int)in.count;
    const uint64_t* src = reinterpret_cast<const uint64_t*>(in.rep);         // a report is six 8-byte words
    uint64_t* dst = reinterpret_cast<uint64_t*>(slot_reports(g.out));
    int done = 0;
    for (int base = 0; base < n; base += AGC_THREADS) {
        const int r = base + tid;
        const bool kept = r < n && g.keep[r] != 0;
        int total;
        const int k = done + block_rank<AGC_WAVES>(kept, total, wsum);
        done += total;
        if (kept) {
            uint64_t w[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) w[q] = src[6 * (size_t)r + q];
#pragma unroll
            for (int q = 0; q < 6; ++q) dst[6 * (size_t)k + q] = w[q];
            if (g.stats) g.stats[r].out_index = k;
        }
    }
    if (tid == 0) slot_close(g.out, (uint32_t)done, false);
}

template <int K> static void launch_stats(const AtiGateArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(atigate_stats_kernel<K>, dim3(a.p.max_detections), dim3(AG_THREADS), 0, st, a);
}

hipError_t launch_atigate(const AtiGateArgs& a, hipStream_t st) {
    const int cells = (2 * (a.p.guard_az + a.p.train_az) + 1) * (2 * (a.p.guard_rg + a.p.train_rg) + 1);
    const int need = (cells + AG_THREADS - 1) / AG_THREADS;
    if (need <= 1) launch_stats<1>(a, st);
    else if (need <= 2) launch_stats<2>(a, st);
    else if (need <= 5) launch_stats<5>(a, st);
    else if (need <= 9) launch_stats<9>(a, st);
    else launch_stats<17>(a, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(atigate_compact_kernel, dim3(1), dim3(AGC_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sarx
