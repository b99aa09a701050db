// GMTI plot extraction (include/sarx_cluster.h has the semantics; tests/_cluster_numpy.py restates them with a flood fill).
//
// One launch, one workgroup of 1024 threads per frame (blockIdx.x = frame), everything of a frame inside its workgroup:
//   labels   : two int32 arrays in LDS, swapped per round (every round reads one and writes the other: no race).  A hook round hands
//              the least label among the reports linked to r to r's root (LDS atomicMin into the array being written); jump rounds
//              (label[r] = label[label[r]]) then flatten the trees completely.  Labels only fall and stay indices of the same
//              component, so the fixed point - every member holds the component's smallest index - does not depend on the order of
//              anything; the loops end when a workgroup-wide __syncthreads_or sees no change, and carry a cap of n + 1 rounds.
//   links    : the list is sorted by (i, j), so the candidates of r in row i' are one contiguous run: a binary search for the key
//              (i', j_r - link_rg), then a walk while j <= j_r + link_rg.  Each search starts where the last one ended and empty rows
//              are stepped over, so a sparse list costs one search per occupied row.  Every index is held inside [0, n).
//   keys     : (i, j) are staged in LDS when the capacity is at most 4096 reports (32 KiB); above that they are read from the slot
//              itself (at most 768 KiB, L2-resident).
//   order    : the keys (label << 14 | index) are sorted in LDS (bitonic): components become contiguous, members in rising index.
//   plots    : the thread at the start of a component walks it for the peak; gmti_dev.hpp's block_rank over the peak flags in
//              report order gives the plot ranks; the thread that owns the peak's index then walks the component again and forms
//              every fp64 value alone, one addition after another.  No global atomics, no scratch, the same bits in every run.
// LDS: 2 x 4 x pow2ceil(capacity) bytes (+ 8 x capacity for the keys): 64 KiB at 4096, 128 KiB at 16384 reports, above the 64 KiB
// a launch gets without asking, hence hipFuncAttributeMaxDynamicSharedMemorySize.
#include "cluster.h"

#include "gmti_dev.hpp"

// the sums must be the restatement's: every fp64 operation rounds on its own
#pragma clang fp contract(off)

namespace sarx {

constexpr int CLUSTER_THREADS = 1024;
constexpr int CLUSTER_WAVES = CLUSTER_THREADS / 64;
constexpr int CLUSTER_LDS_KEYS_MAX = 4096;          // capacities up to this keep (i, j) in LDS
constexpr int INDEX_BITS = 14;                      // SARX_CLUSTER_MAX_DETECTIONS = 1 << 14: label and index share one sort key
constexpr int INDEX_MASK = (1 << INDEX_BITS) - 1;
static_assert(SARX_CLUSTER_MAX_DETECTIONS == 1 << INDEX_BITS, "the sort key holds two 14-bit indices");

template <bool LK> __device__ inline int2 key_at(const sarx_gmti_report* rep, const int2* keys, int s) {
    if (LK) return keys[s];
    return *reinterpret_cast<const int2*>(rep + s);          // i and j lead the record
}

// the least label among r and the reports linked to it; s stays in [0, n) whatever the list holds
template <bool LK>
__device__ inline int least_linked_label(const sarx_gmti_report* rep, const int2* keys, const int* cur, int n, int r, int az, int rg) {
    const int2 kr = key_at<LK>(rep, keys, r);
    int m = cur[r];
    const long long jlo = (long long)kr.y - rg, jhi = (long long)kr.y + rg, last = (long long)kr.x + az;
    long long row = (long long)kr.x - az;
    int pos = 0;
    while (row <= last) {                                    // row rises by one at least: 2 az + 1 rounds at most
        int lo = pos, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int2 k = key_at<LK>(rep, keys, mid);
            if (k.x < row || (k.x == row && k.y < jlo)) lo = mid + 1; else hi = mid;
        }
        int s = lo;
        long long next = row + 1;
        while (s < n) {
            const int2 k = key_at<LK>(rep, keys, s);
            if (k.x != row || k.y > jhi) {
                if (k.x > next) next = k.x;                  // rows without a report are stepped over
                break;
            }
            m = min(m, cur[s]);
            ++s;
        }
        if (s >= n) break;
        pos = s;
        row = next;
    }
    return m;
}

// sixteen waves are four per SIMD: the register budget is that of four, not of the eight the compiler would aim for (it spilt)
template <bool LK>
__global__ __launch_bounds__(CLUSTER_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void cluster_kernel(ClusterArgs a, int pcap) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int wsum[CLUSTER_WAVES];
    int* cur = reinterpret_cast<int*>(smem_raw);             // [pcap]
    int* nxt = cur + pcap;                                   // [pcap]
    int2* keys = reinterpret_cast<int2*>(cur + 2 * (size_t)pcap);      // [max_detections] when LK
    const int tid = threadIdx.x, md = a.p.max_detections;
    const size_t f = blockIdx.x;
    const SlotView in = slot_view(a.in + f * a.in_stride, md);
    const sarx_gmti_report* rep = in.rep;
    char* out_slot = a.out + f * a.out_stride;
    sarx_gmti_report* out = slot_reports(out_slot);
    sarx_cluster_plot* plots = a.plots ? reinterpret_cast<sarx_cluster_plot*>(a.plots + f * a.plots_stride) : nullptr;
    int32_t* labels = a.labels ? a.labels + f * (size_t)md : nullptr;

    if (labels)
        for (int r = tid; r < md; r += CLUSTER_THREADS) labels[r] = -1;
    if (in.unusable || in.count == 0) {
        if (tid == 0) slot_close(out_slot, in.count, in.unusable);
        return;
    }
    const int n = (int)in.count;
    const int az = a.p.link_az, rg = a.p.link_rg;

    for (int r = tid; r < n; r += CLUSTER_THREADS) {
        cur[r] = r;
        if (LK) keys[r] = make_int2(rep[r].i, rep[r].j);
    }
    __syncthreads();

    // ---- labels: hook, then jump until flat; both read `cur` and write `nxt` ----
    // Before a hook round the trees are flat (cur[r] is r's root), so the least label seen by any member is handed to the ROOT, by
    // an LDS atomicMin into the other array: the whole tree follows in the jump rounds, and a label crosses a component in a few
    // rounds however long the way is.  The minimum of a set does not depend on the order of the atomics.
    for (int round = 0; round <= n; ++round) {
        for (int r = tid; r < n; r += CLUSTER_THREADS) nxt[r] = cur[r];
        __syncthreads();
        bool changed = false;
        for (int r = tid; r < n; r += CLUSTER_THREADS) {
            const int m = least_linked_label<LK>(rep, keys, cur, n, r, az, rg);
            if (m < cur[r]) {
                changed = true;
                atomicMin(&nxt[cur[r]], m);
            }
        }
        const int any = __syncthreads_or(changed);
        __syncthreads();
        { int* t = cur; cur = nxt; nxt = t; }
        if (!any) break;
        for (int jump = 0; jump <= n; ++jump) {
            bool moved = false;
            for (int r = tid; r < n; r += CLUSTER_THREADS) {
                const int l = cur[r], m = cur[l];
                moved |= m != l;
                nxt[r] = m;
            }
            const int more = __syncthreads_or(moved);
            __syncthreads();
            { int* t = cur; cur = nxt; nxt = t; }
            if (!more) break;
        }
    }

    // ---- components contiguous, members in rising index: sort (label, index) ----
    int p2 = 1;
    while (p2 < n) p2 <<= 1;                                 // <= pcap
    int* srt = nxt;
    for (int k = tid; k < p2; k += CLUSTER_THREADS) srt[k] = k < n ? ((cur[k] << INDEX_BITS) | k) : 0x7FFFFFFF;
    __syncthreads();
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (p2 >> 1); t += CLUSTER_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const int x = srt[lo], y = srt[hi];
                if ((x > y) == ((lo & size) == 0)) { srt[lo] = y; srt[hi] = x; }
            }
            __syncthreads();
        }
    }

    // ---- the peak of every component that is kept: mark[peak] = 1 + where the component starts in srt ----
    int* mark = cur;
    for (int r = tid; r < n; r += CLUSTER_THREADS) mark[r] = 0;
    __syncthreads();
    for (int k = tid; k < n; k += CLUSTER_THREADS) {
        const int label = srt[k] >> INDEX_BITS;
        if (k > 0 && (srt[k - 1] >> INDEX_BITS) == label) continue;
        int peak = srt[k] & INDEX_MASK;
        double best = rep[peak].power;
        int e = k + 1;
        for (; e < n && (srt[e] >> INDEX_BITS) == label; ++e) {
            const int idx = srt[e] & INDEX_MASK;
            const double pw = rep[idx].power;
            if (pw > best) { best = pw; peak = idx; }
        }
        if (e - k >= a.p.min_members) mark[peak] = k + 1;
    }
    __syncthreads();

    // ---- plots in rising index of their peak; every value of a plot from one thread ----
    int done = 0;
    for (int base = 0; base < n; base += CLUSTER_THREADS) {
        const int r = base + tid;
        const bool is_peak = r < n && mark[r] != 0;
        int total;
        const int k = done + block_rank<CLUSTER_WAVES>(is_peak, total, wsum);
        done += total;
        if (!is_peak) continue;
        const int start = mark[r] - 1, label = srt[start] >> INDEX_BITS;
        const sarx_gmti_report z0 = rep[srt[start] & INDEX_MASK];
        sarx_cluster_plot pl{};
        pl.peak_report = r;
        pl.i_min = pl.i_max = z0.i;
        pl.j_min = pl.j_max = z0.j;
        double sp = z0.power, sre = z0.interf_re, sim = z0.interf_im;
        double wi = z0.power * (double)z0.i, wj = z0.power * (double)z0.j;
        double mr = z0.power / z0.mean;
        if (labels) labels[srt[start] & INDEX_MASK] = k;
        int e = start + 1;
        for (; e < n && (srt[e] >> INDEX_BITS) == label; ++e) {
            const int idx = srt[e] & INDEX_MASK;
            const sarx_gmti_report z = rep[idx];
            pl.i_min = min(pl.i_min, z.i); pl.i_max = max(pl.i_max, z.i);
            pl.j_min = min(pl.j_min, z.j); pl.j_max = max(pl.j_max, z.j);
            sp = sp + z.power; sre = sre + z.interf_re; sim = sim + z.interf_im;
            const double pi = z.power * (double)z.i, pj = z.power * (double)z.j;
            wi = wi + pi; wj = wj + pj;
            const double ratio = z.power / z.mean;
            mr = ratio > mr ? ratio : mr;
            if (labels) labels[idx] = k;
        }
        pl.n_members = e - start;
        pl.sum_power = sp;
        pl.centroid_i = sp == 0.0 ? (double)rep[r].i : wi / sp;
        pl.centroid_j = sp == 0.0 ? (double)rep[r].j : wj / sp;
        pl.max_ratio = mr;
        sarx_gmti_report zp = rep[r];
        zp.interf_re = sre;
        zp.interf_im = sim;
        out[k] = zp;
        if (plots) plots[k] = pl;
    }
    if (tid == 0) slot_close(out_slot, (uint32_t)done, false);
}

static int pow2ceil(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

template <bool LK> static hipError_t launch(const ClusterArgs& a, int n_frames, hipStream_t st) {
    const int pcap = pow2ceil(a.p.max_detections);
    const size_t lds = 2 * (size_t)pcap * sizeof(int) + (LK ? (size_t)a.p.max_detections * sizeof(int2) : 0);
    auto k = cluster_kernel<LK>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(n_frames), dim3(CLUSTER_THREADS), lds, st, a, pcap);
    return hipGetLastError();
}

hipError_t launch_cluster(const ClusterArgs& a, int n_frames, hipStream_t st) {
    return a.p.max_detections <= CLUSTER_LDS_KEYS_MAX ? launch<true>(a, n_frames, st) : launch<false>(a, n_frames, st);
}

}  // namespace sarx
