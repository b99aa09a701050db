// Device-side rules that the kernels of the GMTI chain share (gmti.hip, oscfar.hip, atigate.hip, cluster.hip, track.hip; the
// extent also coherence.hip): the clipped box and its training count, the CFAR tile (geometry, peak rule, bare report,
// launch), the wave and workgroup ranks, and the view of a slot.  Integer and pointer arithmetic, comparisons and conversions
// only: the including files differ in their fp-contract setting, so no floating-point sum or product is formed here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/sarx_gmti.h"

namespace sarx {

// ---- extents: boxes are clipped to the image, so cells outside it are not counted ----
__device__ __forceinline__ int box_extent(int x, int h, int n) { return min(x + h, n - 1) - max(x - h, 0) + 1; }

// cells of the outer box (half-widths oa, orr) around (i, j) that lie outside the guard box (ga, gr)
__device__ __forceinline__ int train_count(int i, int j, int ga, int gr, int oa, int orr, int n_az, int n_rg) {
    return box_extent(i, oa, n_az) * box_extent(j, orr, n_rg) - box_extent(i, ga, n_az) * box_extent(j, gr, n_rg);
}

// ---- CFAR tile: one workgroup of CFAR_THREADS per CFAR_TH x CFAR_TW cells, the tile and its halo in LDS ----
static constexpr int CFAR_TH = 32, CFAR_TW = 64, CFAR_THREADS = 256;

// HA rows / HR columns of halo: the outer half-widths rounded up to 8, 16 or 32.  The fill (K loads, then K LDS stores) is written
// out in each detector: as a shared function it made some CA instantiations slower (profiles/r19_gmti_dev_resource_usage.txt).
template <int HA, int HR> struct CfarTile {
    static constexpr int LH = CFAR_TH + 2 * HA, LW = CFAR_TW + 2 * HR;
    static constexpr int K = LH * LW / CFAR_THREADS;              // loads per thread
    static_assert(LH * LW % CFAR_THREADS == 0, "tile fill: whole loads per thread");
};

// peak rule: whether mc = tile[lr][lc] > 0 is the maximum of its guard box, ties to the smaller index
template <int LW> __device__ __forceinline__ bool guard_box_peak(const float (*tile)[LW], int lr, int lc, float mc, int ga, int gr) {
    for (int di = -ga; di <= ga; ++di)
        for (int dj = -gr; dj <= gr; ++dj) {
            if (!di && !dj) continue;
            const float mq = tile[lr + di][lc + dj];              // zero outside the image: never above mc > 0
            if (mq > mc || (mq == mc && (di < 0 || (di == 0 && dj < 0)))) return false;
        }
    return true;
}

// a detector's report: the interferogram and the magnitudes are the refine launch's to fill in
__device__ __forceinline__ void store_bare_report(sarx_gmti_report* o, int i, int j, double power, double mean) {
    o->i = i;
    o->j = j;
    o->power = power;
    o->mean = mean;
    o->interf_re = 0.0;
    o->interf_im = 0.0;
    o->mag1 = 0.f;
    o->mag2 = 0.f;
}

// Zeroes the header on the stream, then launch(HA, HR, grid) with the halo picked for the outer half-widths oa, orr (HA and HR
// arrive as std::integral_constant: usable as template arguments).
template <class Launch> hipError_t launch_cfar_tiles(sarx_gmti_header* hdr, int n_az, int n_rg, int oa, int orr, hipStream_t st, Launch launch) {
    hipError_t e = hipMemsetAsync(hdr, 0, sizeof(sarx_gmti_header), st);
    if (e != hipSuccess) return e;
    const dim3 grid((n_rg + CFAR_TW - 1) / CFAR_TW, (n_az + CFAR_TH - 1) / CFAR_TH);
    auto range = [&](auto ha) {
        if (orr <= 8) launch(ha, std::integral_constant<int, 8>{}, grid);
        else if (orr <= 16) launch(ha, std::integral_constant<int, 16>{}, grid);
        else launch(ha, std::integral_constant<int, 32>{}, grid);
    };
    if (oa <= 8) range(std::integral_constant<int, 8>{});
    else if (oa <= 16) range(std::integral_constant<int, 16>{});
    else range(std::integral_constant<int, 32>{});
    return hipGetLastError();
}

// ---- ranks ----
// rank of this lane among the flagged lanes of its wave (lane order) and their number
__device__ __forceinline__ unsigned lane_rank(bool flag, unsigned& total) {
    const unsigned long long b = __ballot(flag);
    total = (unsigned)__popcll(b);
    return __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
}

// rank of this thread among the flagged threads of the workgroup of WAVES waves (thread order) and their number
template <int WAVES> __device__ inline int block_rank(bool flag, int& total, int* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned in_wave;
    const int within = (int)lane_rank(flag, in_wave);
    if (lane == 0) wsum[wave] = (int)in_wave;
    __syncthreads();
    int before = 0, tot = 0;
    for (int w = 0; w < WAVES; ++w) {
        const int c = wsum[w];
        tot += c;
        if (w < wave) before += c;
    }
    __syncthreads();
    total = tot;
    return before + within;
}

// ---- slot: the header at the base, the reports behind it ----
struct SlotView {
    const sarx_gmti_report* rep;
    uint32_t count;
    bool unusable;                         // overflowed, or a count beyond the capacity: the list is not to be read
};
__device__ __forceinline__ SlotView slot_view(const void* base, int max_detections) {
    const sarx_gmti_header* hdr = reinterpret_cast<const sarx_gmti_header*>(base);
    SlotView s;
    s.rep = reinterpret_cast<const sarx_gmti_report*>(hdr + 1);
    s.count = hdr->count;
    s.unusable = hdr->overflow != 0 || s.count > (uint32_t)max_detections;
    return s;
}

// where the reports of an output slot go
__device__ __forceinline__ sarx_gmti_report* slot_reports(void* base) {
    return reinterpret_cast<sarx_gmti_report*>(reinterpret_cast<sarx_gmti_header*>(base) + 1);
}
// the header of an output slot (one thread writes it); from an unusable input: its count carried and overflow = 1
__device__ __forceinline__ void slot_close(void* base, uint32_t count, bool overflow) {
    sarx_gmti_header h{};
    h.count = count;
    h.overflow = overflow ? 1u : 0u;
    *reinterpret_cast<sarx_gmti_header*>(base) = h;
}

}  // namespace sarx
