// GMTI tracker kernels (include/sarx_track.h has the semantics; tests/_track_numpy.py restates them in fp64 NumPy).
//
// One step = two launches on one stream:
//   track_pair_kernel    : the nearest-partner searches.  Workgroups [0, nTB) take 256 track slots each and scan the frame's
//                          (i, j), staged in LDS 1024 reports at a time; every lane of a wave reads the same LDS address in the
//                          same cycle (a broadcast, no bank conflict).  Workgroups [nTB, nTB + nRB) do the transposed search, 256
//                          reports each over the predicted positions of the live tracks.  The grid is sized by the capacities;
//                          counts come from the device headers and workgroups without work leave at once.
//   track_resolve_kernel : one workgroup of 1024 threads: matches, updates, status, drops, then the free slots and the births in
//                          order, paired through gmti_dev.hpp's block_rank.  No atomics anywhere: every sum is an integer
//                          count formed in a fixed order, every fp64 value is computed by exactly one thread.
// Both searches form d2 with the same operations on the same operands, so the two sides agree on every pair bit for bit.
#include "track.h"

#include "gmti_dev.hpp"

// the decisions must be the restatement's: every fp64 operation rounds on its own
#pragma clang fp contract(off)

namespace sarx {

constexpr int PAIR_THREADS = 256;
constexpr int PAIR_CHUNK = 1024;           // staged elements: 16 KiB of LDS
constexpr int RESOLVE_THREADS = 1024;
constexpr int RESOLVE_WAVES = RESOLVE_THREADS / 64;

// |d| > gate (1 + 2^-20) gives a quotient above 1 after rounding, a square above 1 and d2 > 1: such a pair is skipped before the
// divisions without changing any decision (a NaN position - a free slot - fails the test as well)
__device__ inline double gate_slack(double g) { return g * (1.0 + 0x1p-20); }

__device__ inline double pair_d2(double di, double dj, double ga, double gr) {
    const double a = di / ga;
    const double b = dj / gr;
    const double aa = a * a;
    const double bb = b * b;
    return aa + bb;
}

__global__ __launch_bounds__(PAIR_THREADS) void track_pair_kernel(TrackArgs a, int n_tb) {
    __shared__ double2 sh[PAIR_CHUNK];
    if (a.hdr->error != SARX_TRACK_OK) return;
    const SlotView in = slot_view(a.slot_hdr, a.p.max_detections);      // count and unusable only: the reports come as a.rep
    if (in.unusable) return;
    const int n = (int)in.count, tid = threadIdx.x;
    const double ga = a.p.gate_az, gr = a.p.gate_rg, sa = gate_slack(ga), sr = gate_slack(gr);
    if ((int)blockIdx.x < n_tb) {
        // ---- tracks over reports ----
        if (a.hdr->n_live == 0) return;
        const int t = blockIdx.x * PAIR_THREADS + tid;
        bool live = false;
        double pi = 0.0, pj = 0.0;
        if (t < a.p.max_tracks && a.slots[t].status != SARX_TRACK_FREE) {
            live = true;
            pi = a.slots[t].p_i + a.slots[t].v_i;
            pj = a.slots[t].p_j + a.slots[t].v_j;
        }
        if (!__syncthreads_or(live)) return;
        int best = -1;
        double bd = __builtin_huge_val();
        for (int base = 0; base < n; base += PAIR_CHUNK) {
            const int m = min(PAIR_CHUNK, n - base);
            __syncthreads();
            for (int k = tid; k < m; k += PAIR_THREADS) sh[k] = make_double2((double)a.rep[base + k].i, (double)a.rep[base + k].j);
            __syncthreads();
            if (live) {
                for (int k = 0; k < m; ++k) {
                    const double2 z = sh[k];
                    const double di = z.x - pi, dj = z.y - pj;
                    if (!(fabs(di) <= sa) || !(fabs(dj) <= sr)) continue;
                    const double d2 = pair_d2(di, dj, ga, gr);
                    if (d2 <= 1.0 && d2 < bd) { bd = d2; best = base + k; }
                }
            }
        }
        if (live) a.best_r[t] = best;
        return;
    }
    // ---- reports over tracks ----
    const int r = ((int)blockIdx.x - n_tb) * PAIR_THREADS + tid;
    if (r - tid >= n) return;
    const bool active = r < n;
    double zi = 0.0, zj = 0.0;
    if (active) { zi = (double)a.rep[r].i; zj = (double)a.rep[r].j; }
    int best = -1;
    double bd = __builtin_huge_val();
    if (a.hdr->n_live != 0) {
        const double nan = __builtin_nan("");
        for (int base = 0; base < a.p.max_tracks; base += PAIR_CHUNK) {
            const int m = min(PAIR_CHUNK, a.p.max_tracks - base);
            __syncthreads();
            bool any = false;
            for (int k = tid; k < m; k += PAIR_THREADS) {
                const sarx_track_slot* s = a.slots + base + k;
                const bool lv = s->status != SARX_TRACK_FREE;
                any |= lv;
                sh[k] = lv ? make_double2(s->p_i + s->v_i, s->p_j + s->v_j) : make_double2(nan, nan);
            }
            if (!__syncthreads_or(any) || !active) continue;
            for (int k = 0; k < m; ++k) {
                const double2 ph = sh[k];
                const double di = zi - ph.x, dj = zj - ph.y;
                if (!(fabs(di) <= sa) || !(fabs(dj) <= sr)) continue;
                const double d2 = pair_d2(di, dj, ga, gr);
                if (d2 <= 1.0 && d2 < bd) { bd = d2; best = base + k; }
            }
        }
    }
    if (active) a.best_t[r] = best;
}

__device__ inline int block_sum(int v, int* wsum) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    int tot = 0;
    for (int w = 0; w < RESOLVE_WAVES; ++w) tot += wsum[w];
    __syncthreads();
    return tot;
}

__device__ inline bool may_start(const sarx_gmti_report& z, double birth_ratio) {
    return birth_ratio == 0.0 || z.power / z.mean >= birth_ratio;
}

__global__ __launch_bounds__(RESOLVE_THREADS) void track_resolve_kernel(TrackArgs a) {
    __shared__ int wsum[RESOLVE_WAVES];
    const int tid = threadIdx.x;
    const sarx_track_header h0 = *a.hdr;
    const SlotView in = slot_view(a.slot_hdr, a.p.max_detections);
    if (h0.error != SARX_TRACK_OK || in.unusable) {
        if (a.assoc)
            for (int r = tid; r < a.p.max_detections; r += RESOLVE_THREADS) a.assoc[r] = -1;
        if (h0.error == SARX_TRACK_OK && tid == 0) {
            a.hdr->error = SARX_TRACK_ERR_SLOT_OVERFLOW;
            a.hdr->error_frame = a.frame;
        }
        return;
    }
    const int n = (int)in.count;
    const bool have_live = h0.n_live != 0;        // without a live track the pair kernel wrote no best_t: every report is unheld

    // the assoc row as "nobody", and how many reports would start a track
    int my_births = 0;
    for (int r = tid; r < a.p.max_detections; r += RESOLVE_THREADS) {
        if (a.assoc) a.assoc[r] = -1;
        if (r < n && (!have_live || a.best_t[r] < 0) && may_start(a.rep[r], a.p.birth_ratio)) ++my_births;
    }
    __syncthreads();

    // matches, updates, status, drops: one thread per slot
    const uint32_t win = a.p.confirm_window >= 32 ? 0xFFFFFFFFu : ((1u << a.p.confirm_window) - 1u);
    int my_live = 0, my_conf = 0, my_drops = 0;
    if (have_live) {
        for (int t = tid; t < a.p.max_tracks; t += RESOLVE_THREADS) {
            sarx_track_slot s = a.slots[t];
            if (s.status == SARX_TRACK_FREE) continue;
            const int r = a.best_r[t];
            const bool matched = r >= 0 && a.best_t[r] == t;
            const double phi = s.p_i + s.v_i, phj = s.p_j + s.v_j;
            if (matched) {
                const sarx_gmti_report z = a.rep[r];
                const double ei = (double)z.i - phi, ej = (double)z.j - phj;
                const double ai = a.p.alpha * ei, aj = a.p.alpha * ej;
                const double bi = a.p.beta * ei, bj = a.p.beta * ej;
                s.p_i = phi + ai; s.p_j = phj + aj;
                s.v_i = s.v_i + bi; s.v_j = s.v_j + bj;
                s.hits += 1; s.misses = 0; s.last_frame = a.frame; s.last_report = r;
                s.sum_re = s.sum_re + z.interf_re; s.sum_im = s.sum_im + z.interf_im; s.sum_power = s.sum_power + z.power;
                const double ratio = z.power / z.mean;
                s.max_ratio = ratio > s.max_ratio ? ratio : s.max_ratio;
                if (a.assoc) a.assoc[r] = s.id;
            } else {
                s.p_i = phi; s.p_j = phj;
                s.misses += 1;
            }
            s.age += 1;
            s.hist = (s.hist << 1) | (matched ? 1u : 0u);
            if (s.status == SARX_TRACK_TENTATIVE && __popc(s.hist & win) >= a.p.confirm_hits) s.status = SARX_TRACK_CONFIRMED;
            if (s.misses > (uint32_t)a.p.max_misses || (s.status == SARX_TRACK_TENTATIVE && s.age >= (uint32_t)a.p.confirm_window)) {
                s = sarx_track_slot{};
                ++my_drops;
            } else {
                ++my_live;
                if (s.status == SARX_TRACK_CONFIRMED) ++my_conf;
            }
            a.slots[t] = s;
        }
    }
    const int births = block_sum(my_births, wsum);
    const int drops = block_sum(my_drops, wsum);
    const int live = block_sum(my_live, wsum);
    const int conf = block_sum(my_conf, wsum);
    const int n_free = a.p.max_tracks - live;
    const bool table_full = births > n_free;

    if (!table_full && births > 0) {
        // the free slots in rising index (each thread reads back the slots it wrote itself) ...
        int done = 0;
        for (int base = 0; base < a.p.max_tracks && done < births; base += RESOLVE_THREADS) {
            const int t = base + tid;
            const bool is_free = t < a.p.max_tracks && a.slots[t].status == SARX_TRACK_FREE;
            int total;
            const int k = done + block_rank<RESOLVE_WAVES>(is_free, total, wsum);
            if (is_free && k < births) a.free_slot[k] = t;
            done += total;
        }
        __threadfence_block();
        __syncthreads();
        // ... and the births in rising report index, the k-th into the k-th free slot
        done = 0;
        for (int base = 0; base < n; base += RESOLVE_THREADS) {
            const int r = base + tid;
            const bool born = r < n && (!have_live || a.best_t[r] < 0) && may_start(a.rep[r], a.p.birth_ratio);
            int total;
            const int k = done + block_rank<RESOLVE_WAVES>(born, total, wsum);
            done += total;
            if (!born) continue;
            const sarx_gmti_report z = a.rep[r];
            sarx_track_slot s{};
            s.p_i = (double)z.i; s.p_j = (double)z.j;
            s.sum_re = z.interf_re; s.sum_im = z.interf_im; s.sum_power = z.power; s.max_ratio = z.power / z.mean;
            s.id = h0.next_id + k;
            s.status = SARX_TRACK_TENTATIVE;
            s.hits = 1; s.age = 1; s.hist = 1u; s.last_frame = a.frame; s.last_report = r;
            a.slots[a.free_slot[k]] = s;
            if (a.assoc) a.assoc[r] = s.id;
        }
    }
    if (tid == 0) {
        sarx_track_header h = h0;
        const int made = table_full ? 0 : births;
        h.n_live = (uint32_t)(live + made);
        h.n_confirmed = (uint32_t)conf;
        h.next_id = h0.next_id + made;
        h.births_total = h0.births_total + (uint32_t)made;
        h.drops_total = h0.drops_total + (uint32_t)drops;
        if (table_full) {
            h.error = SARX_TRACK_ERR_TABLE_OVERFLOW;
            h.error_frame = a.frame;
        } else {
            h.frames_done = h0.frames_done + 1;
        }
        *a.hdr = h;
    }
}

__global__ __launch_bounds__(256) void track_init_kernel(sarx_track_header* hdr, sarx_track_slot* slots, int max_tracks) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < max_tracks) slots[t] = sarx_track_slot{};
    if (t == 0) {
        sarx_track_header h{};
        h.error_frame = -1;
        h.max_tracks = (uint32_t)max_tracks;
        *hdr = h;
    }
}

hipError_t launch_track_init(sarx_track_header* hdr, sarx_track_slot* slots, int max_tracks, hipStream_t st) {
    track_init_kernel<<<(max_tracks + 255) / 256, 256, 0, st>>>(hdr, slots, max_tracks);
    return hipGetLastError();
}

hipError_t launch_track_step(const TrackArgs& a, hipStream_t st) {
    const int n_tb = (a.p.max_tracks + PAIR_THREADS - 1) / PAIR_THREADS;
    const int n_rb = (a.p.max_detections + PAIR_THREADS - 1) / PAIR_THREADS;
    track_pair_kernel<<<n_tb + n_rb, PAIR_THREADS, 0, st>>>(a, n_tb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    track_resolve_kernel<<<1, RESOLVE_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace sarx
