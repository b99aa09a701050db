// Ordered-statistic CFAR on the DPCA magnitude plane (include/sarx_oscfar.h): the launch that stands where gmti.hip's CA launch
// stands and appends to the same list; the refine launch of gmti.hip sorts it.
//
// One workgroup per tile of gmti_dev.hpp, which states the tile's geometry, the peak rule, the report and the ranks for both
// detectors; the tile and its halo are read into LDS as the CA kernel reads them (clamped addresses, every load issued before
// the first wait, zeros outside the image).  The order in which the rules are applied is the reverse of the CA
// kernel's, because here the threshold is the expensive one:
//   1. peak rule, every cell: a cell inside the image with P > 0, N >= min_train that is the maximum of its guard box is a
//      candidate.  Candidates are compacted into an LDS list (ballot + mbcnt prefix, one LDS atomic per wave and pass); the list
//      holds the tile's 2048 cells, so it cannot overflow.
//   2. count, one wave per candidate: the 64 lanes stride over the outer box, each forms alpha * P_t < P in fp64 for its cell when
//      that lies inside the image (by coordinates: an outside cell is skipped, not counted as zero) and outside the guard box, the
//      wave adds the ballots' popcounts.  The loop stops as soon as the count has reached k or can no longer reach it.  No sort,
//      no per-cell array.
//   3. level, one wave per detected cell: x_(k) = the square of the k-th smallest |m_t|, found by bisection on the bit pattern of
//      |m| (for non-negative floats the uint32 order is the value order; the sign bit is masked, so 31 steps), each step the
//      same strided count of #{|m_t| <= v} >= k.
// Each wave takes its slots with one atomic on the header's count.  alpha * P_t is a product of two factors and P_t = m * m is
// exact in fp64: there is no multiply-add to contract and nothing to reassociate in these expressions.
#include "oscfar.h"

#include "gmti_dev.hpp"

namespace sarx {

static constexpr int OS_WAVES = CFAR_THREADS / 64;
static constexpr int OS_CELLS = CFAR_TH * CFAR_TW;
static constexpr int OS_PER_THREAD = OS_CELLS / CFAR_THREADS;
static constexpr unsigned short OS_DETECTED = 0x8000;             // flag on a candidate's tile index (< OS_CELLS = 2048)

struct OsCell {
    int lr, lc;                  // tile coordinates of the cell under test
    int gi, gj;                  // image coordinates
    int k;                       // the rank scaled to the cell's training count: the k-th smallest is its level
};

// the candidate with tile index `cell` of the tile at (r0, c0)
template <int HA, int HR> __device__ __forceinline__ OsCell os_cell(const OsCfarArgs& args, int r0, int c0, int cell) {
    const GmtiCfarArgs& a = args.base;
    OsCell c;
    c.lr = cell / CFAR_TW + HA; c.lc = cell % CFAR_TW + HR; c.gi = r0 + cell / CFAR_TW; c.gj = c0 + cell % CFAR_TW;
    const int n_train = train_count(c.gi, c.gj, a.ga, a.gr, a.oa, a.orr, a.n_az, a.n_rg);
    c.k = (args.rank * n_train + args.n_full - 1) / args.n_full;
    return c;
}

// Whether at least `need` training cells of `c` satisfy pred(m_t).  Wave-uniform: every lane returns the same answer.
template <int LW, class Pred>
__device__ __forceinline__ bool os_count_reaches(const float (*tile)[LW], const GmtiCfarArgs& a, const OsCell& c, int lane, int need,
                                                 Pred pred) {
    const int W = 2 * a.orr + 1, total = (2 * a.oa + 1) * W;
    const int step_i = 64 / W, step_j = 64 % W;
    int di = lane / W, dj = lane % W;                             // from the outer box's first row and column
    int cnt = 0;
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int ai = di - a.oa, aj = dj - a.orr;
        const bool in = t0 + lane < total && (unsigned)(c.gi + ai) < (unsigned)a.n_az && (unsigned)(c.gj + aj) < (unsigned)a.n_rg &&
                        !(abs(ai) <= a.ga && abs(aj) <= a.gr);
        bool hit = false;
        if (in) hit = pred(tile[c.lr + ai][c.lc + aj]);
        cnt += (int)__popcll(__ballot(hit));
        if (cnt >= need || cnt + (total - t0 - 64) < need) break;
        di += step_i;
        dj += step_j;
        if (dj >= W) { dj -= W; ++di; }
    }
    return cnt >= need;
}

template <int HA, int HR> __global__ __launch_bounds__(CFAR_THREADS) void gmti_oscfar_kernel(OsCfarArgs args) {
    using Tile = CfarTile<HA, HR>;
    constexpr int LH = Tile::LH, LW = Tile::LW, K = Tile::K;
    __shared__ float tile[LH][LW];
    __shared__ unsigned short cand[OS_CELLS];
    __shared__ unsigned n_cand;
    const GmtiCfarArgs& a = args.base;
    const int r0 = blockIdx.y * CFAR_TH, c0 = blockIdx.x * CFAR_TW;
    const int tid = threadIdx.x, lane = tid & 63;

    // tile fill, as in gmti.hip: clamped addresses (always a valid load), zero outside the image afterwards
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * CFAR_THREADS;
        const int gr = r0 - HA + e / LW, gc = c0 - HR + e % LW;
        const int cr = min(max(gr, 0), a.n_az - 1), cc = min(max(gc, 0), a.n_rg - 1);
        v[k] = a.m[(size_t)cr * a.n_rg + cc];
    }
    __builtin_amdgcn_sched_barrier(0);                            // every load is issued before the first is waited for
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * CFAR_THREADS;
        const int gr = r0 - HA + e / LW, gc = c0 - HR + e % LW;
        const bool inside = (unsigned)gr < (unsigned)a.n_az && (unsigned)gc < (unsigned)a.n_rg;
        tile[e / LW][e % LW] = inside ? v[k] : 0.f;
    }
    if (tid == 0) n_cand = 0;
    __syncthreads();

    // 1. candidates: a wave takes one tile row of 64 cells per pass (consecutive LDS addresses)
#pragma unroll 1
    for (int q = 0; q < OS_PER_THREAD; ++q) {
        const int e = tid + q * CFAR_THREADS;
        const int r = e / CFAR_TW, c = e % CFAR_TW;
        const int gi = r0 + r, gj = c0 + c, lr = r + HA, lc = c + HR;
        const float mc = tile[lr][lc];
        const int n_train = train_count(gi, gj, a.ga, a.gr, a.oa, a.orr, a.n_az, a.n_rg);
        bool is = gi < a.n_az && gj < a.n_rg && n_train >= a.min_train && (double)mc * (double)mc > 0.0;
        if (is) is = guard_box_peak<LW>(tile, lr, lc, mc, a.ga, a.gr);      // a branch, not one && chain: mc stays loaded before the tests
        unsigned found;
        const unsigned within = lane_rank(is, found);
        if (found == 0) continue;                                 // wave-uniform
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&n_cand, found);
        base = __shfl(base, 0);
        if (is) cand[base + within] = (unsigned short)e;
    }
    __syncthreads();

    // 2. the count decides; a detected candidate is flagged in place (the wave that flags an entry is the one that reads it again,
    // and all its lanes store the same value)
    const int nc = (int)n_cand, wave = tid / 64;
    unsigned mine = 0;
    for (int idx = wave; idx < nc; idx += OS_WAVES) {
        const int e = cand[idx];
        const OsCell c = os_cell<HA, HR>(args, r0, c0, e);
        const float mc = tile[c.lr][c.lc];
        const double p = (double)mc * (double)mc, alpha = a.alpha;
        if (os_count_reaches<LW>(tile, a, c, lane, c.k, [=](float x) { return alpha * ((double)x * (double)x) < p; })) {
            cand[idx] = (unsigned short)(e | OS_DETECTED);
            ++mine;
        }
    }
    if (mine == 0) return;                                        // wave-uniform

    // 3. the wave's reports get consecutive slots from one atomic; the level of each by bisection
    unsigned slot = 0;
    if (lane == 0) {
        slot = atomicAdd(&a.hdr->count, mine);
        if (slot + mine > (unsigned)a.max_det) atomicOr(&a.hdr->overflow, 1u);
    }
    slot = __shfl(slot, 0);
    for (int idx = wave; idx < nc; idx += OS_WAVES) {
        const int e = cand[idx];
        if (!(e & OS_DETECTED)) continue;                         // wave-uniform
        if (slot >= (unsigned)a.max_det) return;                  // overflowed: the list is an error, nothing more to write
        const OsCell c = os_cell<HA, HR>(args, r0, c0, e & (OS_CELLS - 1));
        unsigned bits = 0;                                        // the smallest v with #{|m_t| <= v} >= k is the k-th smallest |m_t|
        for (int b = 30; b >= 0; --b) {
            const unsigned trial = bits | ((1u << b) - 1u);
            if (!os_count_reaches<LW>(tile, a, c, lane, c.k, [=](float x) { return (__float_as_uint(x) & 0x7fffffffu) <= trial; })) bits |= 1u << b;
        }
        if (lane == 0) {
            const float mc = tile[c.lr][c.lc], mk = __uint_as_float(bits);
            store_bare_report(a.rep + slot, c.gi, c.gj, (double)mc * (double)mc, (double)mk * (double)mk);
        }
        ++slot;
    }
}

hipError_t launch_gmti_oscfar(const OsCfarArgs& a, hipStream_t st) {
    const GmtiCfarArgs& b = a.base;
    return launch_cfar_tiles(b.hdr, b.n_az, b.n_rg, b.oa, b.orr, st, [&](auto ha, auto hr, dim3 grid) {
        hipLaunchKernelGGL((gmti_oscfar_kernel<ha(), hr()>), grid, dim3(CFAR_THREADS), 0, st, a);
    });
}

}  // namespace sarx
