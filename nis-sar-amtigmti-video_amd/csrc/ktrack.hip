// Kalman ground tracker kernels (include/sarx_ktrack.h has the semantics; tests/_ktrack_numpy.py restates them in fp64 NumPy).
//
// One step = four launches on one stream, built like track.hip:
//   ktrack_prepare_kernel : one lane per track slot writes the prediction x-, P- (14 doubles), one lane per report z, u and Rm (11
//                           doubles) to the workspace, one plane per value so that the loads below coalesce.  A free slot, a
//                           report that is no measurement and the padding up to a whole stage get a NaN in plane 0: they fail the
//                           coarse gate.
//   ktrack_pair_kernel    : the nearest-partner searches.  Workgroups [0, nTB) take 256 track slots each and scan the frame's
//                           measurements, staged in LDS 256 at a time (11 planes, 22 KiB); every lane of a wave reads the same LDS
//                           address in the same cycle (a broadcast, no bank conflict).  Workgroups [nTB, nTB + nRB) do the
//                           transposed search, 256 reports each over the predictions (14 planes, 28 KiB).  Stages have a fixed
//                           length.  Both searches call ktrack_innov on the same operands, so the two sides agree on every pair's
//                           d2 bit for bit: that is what makes mutual nearest neighbour well defined.
//   ktrack_update_kernel  : one lane per matched track: ktrack_innov again, then the gain and the Joseph form; the posterior takes
//                           the prediction's place in the workspace, d2 goes to a plane of its own.  A launch of its own because
//                           inside the 1024-thread resolve workgroup (128 VGPRs per lane) the 4 x 4 update spilled 248 bytes per
//                           lane to scratch; with 256 threads it has the registers it needs.
//   ktrack_resolve_kernel : one workgroup of 1024 threads: matches, the states taken from the workspace, counters, status, drops,
//                           then the free slots and the births in order, paired through gmti_dev.hpp's block_rank.
// The grids are sized by the capacities; counts come from the device headers and workgroups without work leave at once.  No atomics:
// every sum is an integer count formed in a fixed order, every fp64 value is computed by exactly one thread.
#include "ktrack.h"

#include "gmti_dev.hpp"

// the decisions must be the restatement's: every fp64 operation rounds on its own
#pragma clang fp contract(off)

namespace sarx {

constexpr int KT_THREADS = KTRACK_STAGE;
constexpr int KT_RESOLVE_THREADS = 1024;
constexpr int KT_RESOLVE_WAVES = KT_RESOLVE_THREADS / 64;

struct KStep { bool go; uint32_t err; int n; double dt; };

// steps 1a - 1c of the header, evaluated alike by every thread of the four launches (the header is written by the resolve launch's
// last act only)
__device__ inline KStep ktrack_step_state(const KtrackArgs& a) {
    KStep s{false, SARX_KTRACK_OK, 0, 0.0};
    if (a.hdr->error != SARX_KTRACK_OK) return s;
    const SlotView in = slot_view(a.slot_hdr, a.p.max_detections);
    if (in.unusable || (in.count >= 1u && a.rec[0].status == SARX_RELOCATE_OVERFLOW)) { s.err = SARX_KTRACK_ERR_SLOT_OVERFLOW; return s; }
    s.n = (int)in.count;
    s.dt = a.hdr->frames_done == 0u ? 0.0 : a.f.t - a.hdr->t_last;
    if (!(s.dt >= 0.0) || !(s.dt <= 1.7976931348623157e308)) { s.err = SARX_KTRACK_ERR_TIME; return s; }
    s.go = true;
    return s;
}

struct KPred { double x[4]; double p[10]; };                       // x-, y-, vx-, vy-; the upper triangle of P-
struct KMeas { double z[3]; double ux, uy; double r00, r01, r11, r02, r12, r22; };
struct KInnov { double nu[3]; double c[4]; double l00, l10, l20, l11, l21, l22; double d2; };

// index of P[i][j] in the upper triangle
__device__ __forceinline__ constexpr int kp(int i, int j) { return i <= j ? i * 4 - i * (i - 1) / 2 + (j - i) : j * 4 - j * (j - 1) / 2 + (i - j); }

// step 4 of the header: false when the pair fails the coarse box (nothing else is then formed); d2 may be NaN
__device__ __forceinline__ bool ktrack_innov(const KPred& t, const KMeas& m, double gate_m, KInnov& o) {
    o.nu[0] = m.z[0] - t.x[0];
    if (!(fabs(o.nu[0]) <= gate_m)) return false;
    o.nu[1] = m.z[1] - t.x[1];
    if (!(fabs(o.nu[1]) <= gate_m)) return false;
    o.nu[2] = m.z[2] - (m.ux * t.x[2] + m.uy * t.x[3]);
    o.c[0] = m.ux * t.p[2] + m.uy * t.p[3];
    o.c[1] = m.ux * t.p[5] + m.uy * t.p[6];
    o.c[2] = m.ux * t.p[7] + m.uy * t.p[8];
    o.c[3] = m.ux * t.p[8] + m.uy * t.p[9];
    const double s00 = t.p[0] + m.r00, s01 = t.p[1] + m.r01, s11 = t.p[4] + m.r11;
    const double s02 = o.c[0] + m.r02, s12 = o.c[1] + m.r12;
    const double s22 = (m.ux * o.c[2] + m.uy * o.c[3]) + m.r22;
    o.l00 = sqrt(s00);
    o.l10 = s01 / o.l00;
    o.l20 = s02 / o.l00;
    o.l11 = sqrt(s11 - o.l10 * o.l10);
    o.l21 = (s12 - o.l20 * o.l10) / o.l11;
    o.l22 = sqrt((s22 - o.l20 * o.l20) - o.l21 * o.l21);
    const double w0 = o.nu[0] / o.l00;
    const double w1 = (o.nu[1] - o.l10 * w0) / o.l11;
    const double w2 = ((o.nu[2] - o.l20 * w0) - o.l21 * w1) / o.l22;
    o.d2 = (w0 * w0 + w1 * w1) + w2 * w2;
    return true;
}

__device__ __forceinline__ KPred load_pred(const double* pred, int tp, int t) {
    KPred k;
#pragma unroll
    for (int f = 0; f < 4; ++f) k.x[f] = pred[(size_t)f * tp + t];
#pragma unroll
    for (int f = 0; f < 10; ++f) k.p[f] = pred[(size_t)(4 + f) * tp + t];
    return k;
}
__device__ __forceinline__ KMeas load_meas(const double* meas, int rp, int r) {
    KMeas m;
    m.z[0] = meas[r]; m.z[1] = meas[(size_t)rp + r]; m.z[2] = meas[(size_t)2 * rp + r];
    m.ux = meas[(size_t)3 * rp + r]; m.uy = meas[(size_t)4 * rp + r];
    m.r00 = meas[(size_t)5 * rp + r]; m.r01 = meas[(size_t)6 * rp + r]; m.r11 = meas[(size_t)7 * rp + r];
    m.r02 = meas[(size_t)8 * rp + r]; m.r12 = meas[(size_t)9 * rp + r]; m.r22 = meas[(size_t)10 * rp + r];
    return m;
}

// ---- prepare -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KT_THREADS) void ktrack_prepare_kernel(KtrackArgs a, int n_tb) {
    const KStep st = ktrack_step_state(a);
    if (!st.go) return;
    const int tid = threadIdx.x;
    const double nan = __builtin_nan("");
    if ((int)blockIdx.x < n_tb) {
        // ---- step 2: one lane per track slot, the padding included ----
        if (a.hdr->n_live == 0) return;
        const int t = blockIdx.x * KT_THREADS + tid;                 // < tp
        double* o = a.pred + t;
        if (t >= a.p.max_tracks || a.slots[t].status == SARX_KTRACK_FREE) { o[0] = nan; return; }
        const sarx_ktrack_slot s = a.slots[t];
        const double dt = st.dt, dt2 = dt * dt, dt3 = dt2 * dt;
        const double q11 = a.p.q * (dt3 / 3.0), q13 = a.p.q * (dt2 / 2.0), q33 = a.p.q * dt;
        const double* P = s.p;
        const size_t tp = (size_t)a.tp;
        o[0] = s.x + dt * s.vx;
        o[tp] = s.y + dt * s.vy;
        o[2 * tp] = s.vx;
        o[3 * tp] = s.vy;
        o[4 * tp] = P[0] + dt * (P[2] + P[2]) + dt2 * P[7] + q11;
        o[5 * tp] = P[1] + dt * (P[3] + P[5]) + dt2 * P[8];
        o[6 * tp] = P[2] + dt * P[7] + q13;
        o[7 * tp] = P[3] + dt * P[8];
        o[8 * tp] = P[4] + dt * (P[6] + P[6]) + dt2 * P[9] + q11;
        o[9 * tp] = P[5] + dt * P[8];
        o[10 * tp] = P[6] + dt * P[9] + q13;
        o[11 * tp] = P[7] + q33;
        o[12 * tp] = P[8];
        o[13 * tp] = P[9] + q33;
        return;
    }
    // ---- step 3: one lane per report, up to the end of the last stage that holds one ----
    const int r = ((int)blockIdx.x - n_tb) * KT_THREADS + tid;      // < rp
    if (r - tid >= st.n) return;
    double* o = a.meas + r;
    if (r >= st.n) { o[0] = nan; return; }
    const sarx_relocate_record rec = a.rec[r];
    const double v = *(const double*)(a.v_los + (size_t)r * a.v_los_stride);
    const double Vx = a.f.vel_ref[0], Vy = a.f.vel_ref[1];
    const double s = sqrt(Vx * Vx + Vy * Vy);
    const double dx = rec.x - a.f.pos_ref[0], dy = rec.y - a.f.pos_ref[1];
    const double rho2 = dx * dx + dy * dy;
    const bool solved = rec.status == SARX_RELOCATE_OK || rec.status == SARX_RELOCATE_OFF_GRID;
    if (!solved || !(fabs(v) <= 1.7976931348623157e308) || !(fabs(rec.x) <= 1.7976931348623157e308) ||
        !(fabs(rec.y) <= 1.7976931348623157e308) || s == 0.0 || rho2 == 0.0) {
        o[0] = nan;
        return;
    }
    const double ax = Vx / s, ay = Vy / s, nx = -ay, ny = ax;
    const double R = sqrt(rho2 + a.f.pos_ref[2] * a.f.pos_ref[2]);
    const double k = R / s, kax = k * ax, kay = k * ay;
    const double sp2 = a.p.sigma_pos * a.p.sigma_pos, sv2 = a.p.sigma_v * a.p.sigma_v;
    const size_t rp = (size_t)a.rp;
    o[0] = rec.x;
    o[rp] = rec.y;
    o[2 * rp] = v;
    o[3 * rp] = dx / R;
    o[4 * rp] = dy / R;
    o[5 * rp] = (ax * ax) * sp2 + (nx * nx) * sp2 + (kax * kax) * sv2;
    o[6 * rp] = (ax * ay) * sp2 + (nx * ny) * sp2 + (kax * kay) * sv2;
    o[7 * rp] = (ay * ay) * sp2 + (ny * ny) * sp2 + (kay * kay) * sv2;
    o[8 * rp] = kax * sv2;
    o[9 * rp] = kay * sv2;
    o[10 * rp] = sv2;
}

// ---- pair ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KT_THREADS) void ktrack_pair_kernel(KtrackArgs a, int n_tb) {
    __shared__ double sh[KTRACK_PRED * KTRACK_STAGE];
    const KStep st = ktrack_step_state(a);
    if (!st.go) return;
    const int n = st.n, tid = threadIdx.x;
    const double gm = a.p.gate_m, gd = a.p.gate_d2;
    if (a.hdr->n_live == 0) return;                                  // nobody reads best_r or best_t then
    if ((int)blockIdx.x < n_tb) {
        // ---- tracks over measurements ----
        const int t = blockIdx.x * KT_THREADS + tid;
        const bool live = t < a.p.max_tracks && a.slots[t].status != SARX_KTRACK_FREE;
        if (!__syncthreads_or(live)) return;
        KPred me{};
        if (live) me = load_pred(a.pred, a.tp, t);
        int best = -1;
        double bd = __builtin_huge_val();
        for (int base = 0; base < n; base += KTRACK_STAGE) {
            __syncthreads();
#pragma unroll
            for (int f = 0; f < KTRACK_MEAS; ++f) sh[f * KTRACK_STAGE + tid] = a.meas[(size_t)f * a.rp + base + tid];
            __syncthreads();
            if (live) {
                for (int k = 0; k < KTRACK_STAGE; ++k) {
                    KMeas m;
                    m.z[0] = sh[k];
                    if (!(fabs(m.z[0] - me.x[0]) <= gm)) continue;
                    m.z[1] = sh[KTRACK_STAGE + k]; m.z[2] = sh[2 * KTRACK_STAGE + k];
                    m.ux = sh[3 * KTRACK_STAGE + k]; m.uy = sh[4 * KTRACK_STAGE + k];
                    m.r00 = sh[5 * KTRACK_STAGE + k]; m.r01 = sh[6 * KTRACK_STAGE + k]; m.r11 = sh[7 * KTRACK_STAGE + k];
                    m.r02 = sh[8 * KTRACK_STAGE + k]; m.r12 = sh[9 * KTRACK_STAGE + k]; m.r22 = sh[10 * KTRACK_STAGE + k];
                    KInnov in;
                    if (!ktrack_innov(me, m, gm, in)) continue;
                    if (in.d2 <= gd && in.d2 < bd) { bd = in.d2; best = base + k; }
                }
            }
        }
        if (live) a.best_r[t] = best;
        return;
    }
    // ---- measurements over tracks ----
    const int r = ((int)blockIdx.x - n_tb) * KT_THREADS + tid;
    if (r - tid >= n) return;
    const bool mine = r < n;
    KMeas me{};
    if (mine) me = load_meas(a.meas, a.rp, r);
    const bool active = mine && me.z[0] == me.z[0];
    int best = -1;
    double bd = __builtin_huge_val();
    for (int base = 0; base < a.tp; base += KTRACK_STAGE) {
        __syncthreads();
        const double x0 = a.pred[base + tid];
        sh[tid] = x0;
        if (!__syncthreads_or(x0 == x0)) continue;                   // a stage of free slots
#pragma unroll
        for (int f = 1; f < KTRACK_PRED; ++f) sh[f * KTRACK_STAGE + tid] = a.pred[(size_t)f * a.tp + base + tid];
        __syncthreads();
        if (!active) continue;
        for (int k = 0; k < KTRACK_STAGE; ++k) {
            KPred t;
            t.x[0] = sh[k];
            if (!(fabs(me.z[0] - t.x[0]) <= gm)) continue;
#pragma unroll
            for (int f = 1; f < 4; ++f) t.x[f] = sh[f * KTRACK_STAGE + k];
#pragma unroll
            for (int f = 0; f < 10; ++f) t.p[f] = sh[(4 + f) * KTRACK_STAGE + k];
            KInnov in;
            if (!ktrack_innov(t, me, gm, in)) continue;
            if (in.d2 <= gd && in.d2 < bd) { bd = in.d2; best = base + k; }
        }
    }
    if (mine) a.best_t[r] = best;
}

// ---- resolve -------------------------------------------------------------------------------------------------------------------------
__device__ inline int kt_block_sum(int v, int* wsum) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    int tot = 0;
    for (int w = 0; w < KT_RESOLVE_WAVES; ++w) tot += wsum[w];
    __syncthreads();
    return tot;
}

// step 6 of the header: the state and P of a matched track from its prediction, the measurement and their innovation
__device__ __forceinline__ void ktrack_update(const KPred& t, const KMeas& m, const KInnov& in, KPred& s) {
    const double rm[3][3] = {{m.r00, m.r01, m.r02}, {m.r01, m.r11, m.r12}, {m.r02, m.r12, m.r22}};
    double K[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double b0 = t.p[kp(i, 0)], b1 = t.p[kp(i, 1)], b2 = in.c[i];
        const double y0 = b0 / in.l00;
        const double y1 = (b1 - in.l10 * y0) / in.l11;
        const double y2 = ((b2 - in.l20 * y0) - in.l21 * y1) / in.l22;
        K[i][2] = y2 / in.l22;
        K[i][1] = (y1 - in.l21 * K[i][2]) / in.l11;
        K[i][0] = ((y0 - in.l10 * K[i][1]) - in.l20 * K[i][2]) / in.l00;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s.x[i] = t.x[i] + ((K[i][0] * in.nu[0] + K[i][1] * in.nu[1]) + K[i][2] * in.nu[2]);
    double A[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        A[i][0] = (i == 0 ? 1.0 : 0.0) - K[i][0];
        A[i][1] = (i == 1 ? 1.0 : 0.0) - K[i][1];
        A[i][2] = (i == 2 ? 1.0 : 0.0) - K[i][2] * m.ux;
        A[i][3] = (i == 3 ? 1.0 : 0.0) - K[i][2] * m.uy;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double M[4], G[3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            M[j] = ((A[i][0] * t.p[kp(0, j)] + A[i][1] * t.p[kp(1, j)]) + A[i][2] * t.p[kp(2, j)]) + A[i][3] * t.p[kp(3, j)];
#pragma unroll
        for (int c = 0; c < 3; ++c) G[c] = (K[i][0] * rm[0][c] + K[i][1] * rm[1][c]) + K[i][2] * rm[2][c];
#pragma unroll
        for (int j = i; j < 4; ++j) {
            const double T = ((M[0] * A[j][0] + M[1] * A[j][1]) + M[2] * A[j][2]) + M[3] * A[j][3];
            const double U = (G[0] * K[j][0] + G[1] * K[j][1]) + G[2] * K[j][2];
            s.p[kp(i, j)] = T + U;
        }
    }
}

// whether track slot t (live) and its best measurement chose each other; r = that measurement
__device__ __forceinline__ bool kt_matched(const KtrackArgs& a, int t, int n, int& r) {
    r = a.best_r[t];
    return r >= 0 && r < n && a.best_t[r] == t;
}

__global__ __launch_bounds__(KT_THREADS) void ktrack_update_kernel(KtrackArgs a) {
    const KStep st = ktrack_step_state(a);
    if (!st.go || a.hdr->n_live == 0) return;
    const int t = blockIdx.x * KT_THREADS + threadIdx.x;
    if (t >= a.p.max_tracks || a.slots[t].status == SARX_KTRACK_FREE) return;
    int r;
    if (!kt_matched(a, t, st.n, r)) return;
    const KPred pr = load_pred(a.pred, a.tp, t);
    const KMeas m = load_meas(a.meas, a.rp, r);
    KInnov in;
    if (!ktrack_innov(pr, m, a.p.gate_m, in)) return;               // never: the pair launch found the pair eligible
    KPred post;
    ktrack_update(pr, m, in, post);
    const size_t tp = (size_t)a.tp;
#pragma unroll
    for (int f = 0; f < 4; ++f) a.pred[f * tp + t] = post.x[f];
#pragma unroll
    for (int f = 0; f < 10; ++f) a.pred[(4 + f) * tp + t] = post.p[f];
    a.nis[t] = in.d2;
}

__device__ inline bool kt_may_start(const sarx_gmti_report& z, double birth_ratio) {
    return birth_ratio == 0.0 || z.power / z.mean >= birth_ratio;
}

__global__ __launch_bounds__(KT_RESOLVE_THREADS) void ktrack_resolve_kernel(KtrackArgs a) {
    __shared__ int wsum[KT_RESOLVE_WAVES];
    const int tid = threadIdx.x;
    const sarx_ktrack_header h0 = *a.hdr;
    const KStep st = ktrack_step_state(a);
    __syncthreads();                                                 // every thread has read the header before thread 0 writes it
    if (!st.go) {
        if (a.assoc)
            for (int r = tid; r < a.p.max_detections; r += KT_RESOLVE_THREADS) a.assoc[r] = -1;
        if (st.err != SARX_KTRACK_OK && tid == 0) {
            a.hdr->error = st.err;
            a.hdr->error_frame = a.f.frame_index;
        }
        return;
    }
    const int n = st.n;
    const bool have_live = h0.n_live != 0;        // without a live track the pair launch wrote no best_t: every measurement is unheld

    // the assoc row as "nobody", and how many measurements would start a track
    int my_births = 0;
    for (int r = tid; r < a.p.max_detections; r += KT_RESOLVE_THREADS) {
        if (a.assoc) a.assoc[r] = -1;
        if (r < n && a.meas[r] == a.meas[r] && (!have_live || a.best_t[r] < 0) && kt_may_start(a.rep[r], a.p.birth_ratio)) ++my_births;
    }
    __syncthreads();

    // matches, updates, status, drops: one thread per slot
    const uint32_t win = a.p.confirm_window >= 32 ? 0xFFFFFFFFu : ((1u << a.p.confirm_window) - 1u);
    int my_live = 0, my_conf = 0, my_drops = 0;
    if (have_live) {
        for (int t = tid; t < a.p.max_tracks; t += KT_RESOLVE_THREADS) {
            if (a.slots[t].status == SARX_KTRACK_FREE) continue;
            sarx_ktrack_slot s = a.slots[t];
            int r;
            const bool updated = kt_matched(a, t, n, r);
            const KPred pr = load_pred(a.pred, a.tp, t);             // the posterior where the update launch wrote one
            s.x = pr.x[0]; s.y = pr.x[1]; s.vx = pr.x[2]; s.vy = pr.x[3];
#pragma unroll
            for (int f = 0; f < 10; ++f) s.p[f] = pr.p[f];
            if (updated) {
                const sarx_gmti_report z = a.rep[r];
                const double d2 = a.nis[t];
                s.nis_last = d2;
                s.nis_sum = s.nis_sum + d2;
                s.hits += 1; s.misses = 0; s.last_frame = a.f.frame_index; s.last_report = r;
                s.sum_re = s.sum_re + z.interf_re; s.sum_im = s.sum_im + z.interf_im; s.sum_power = s.sum_power + z.power;
                const double ratio = z.power / z.mean;
                s.max_ratio = ratio > s.max_ratio ? ratio : s.max_ratio;
                if (a.assoc) a.assoc[r] = s.id;
            } else {
                s.misses += 1;
            }
            s.age += 1;
            s.hist = (s.hist << 1) | (updated ? 1u : 0u);
            if (s.status == SARX_KTRACK_TENTATIVE && __popc(s.hist & win) >= a.p.confirm_hits) s.status = SARX_KTRACK_CONFIRMED;
            if (s.misses > (uint32_t)a.p.max_misses || (s.status == SARX_KTRACK_TENTATIVE && s.age >= (uint32_t)a.p.confirm_window)) {
                s = sarx_ktrack_slot{};
                ++my_drops;
            } else {
                ++my_live;
                if (s.status == SARX_KTRACK_CONFIRMED) ++my_conf;
            }
            a.slots[t] = s;
        }
    }
    const int births = kt_block_sum(my_births, wsum);
    const int drops = kt_block_sum(my_drops, wsum);
    const int live = kt_block_sum(my_live, wsum);
    const int conf = kt_block_sum(my_conf, wsum);
    const int n_free = a.p.max_tracks - live;
    const bool table_full = births > n_free;

    if (!table_full && births > 0) {
        // the free slots in rising index (each thread reads back the slots it wrote itself) ...
        int done = 0;
        for (int base = 0; base < a.p.max_tracks && done < births; base += KT_RESOLVE_THREADS) {
            const int t = base + tid;
            const bool is_free = t < a.p.max_tracks && a.slots[t].status == SARX_KTRACK_FREE;
            int total;
            const int k = done + block_rank<KT_RESOLVE_WAVES>(is_free, total, wsum);
            if (is_free && k < births) a.free_slot[k] = t;
            done += total;
        }
        __threadfence_block();
        __syncthreads();
        // ... and the births in rising report index, the k-th into the k-th free slot (step 9 of the header)
        done = 0;
        for (int base = 0; base < n; base += KT_RESOLVE_THREADS) {
            const int r = base + tid;
            const bool born = r < n && a.meas[r] == a.meas[r] && (!have_live || a.best_t[r] < 0) && kt_may_start(a.rep[r], a.p.birth_ratio);
            int total;
            const int k = done + block_rank<KT_RESOLVE_WAVES>(born, total, wsum);
            done += total;
            if (!born) continue;
            const sarx_gmti_report z = a.rep[r];
            const KMeas m = load_meas(a.meas, a.rp, r);
            sarx_ktrack_slot s{};
            const double mm = sqrt(m.ux * m.ux + m.uy * m.uy);
            const double ex = m.ux / mm, ey = m.uy / mm, emx = ex / mm, emy = ey / mm, tx = -ey, ty = ex;
            s.x = m.z[0]; s.y = m.z[1];
            s.p[0] = m.r00; s.p[1] = m.r01; s.p[4] = m.r11;
            s.p[2] = m.r02 * emx; s.p[3] = m.r02 * emy; s.p[5] = m.r12 * emx; s.p[6] = m.r12 * emy;
            if (a.rec[r].flags & SARX_RELOCATE_HAS_VELOCITY) {
                s.vx = a.rec[r].vx; s.vy = a.rec[r].vy;
                s.p[7] = m.r22; s.p[8] = 0.0; s.p[9] = m.r22;
            } else {
                const double vr = m.z[2] / mm;
                s.vx = vr * ex; s.vy = vr * ey;
                const double sm = a.p.sigma_v / mm, sm2 = sm * sm, st2 = a.p.sigma_v_tan * a.p.sigma_v_tan;
                s.p[7] = sm2 * (ex * ex) + st2 * (tx * tx);
                s.p[8] = sm2 * (ex * ey) + st2 * (tx * ty);
                s.p[9] = sm2 * (ey * ey) + st2 * (ty * ty);
            }
            s.sum_re = z.interf_re; s.sum_im = z.interf_im; s.sum_power = z.power; s.max_ratio = z.power / z.mean;
            s.id = h0.next_id + k;
            s.status = SARX_KTRACK_TENTATIVE;
            s.hits = 1; s.age = 1; s.hist = 1u; s.last_frame = a.f.frame_index; s.last_report = r;
            a.slots[a.free_slot[k]] = s;
            if (a.assoc) a.assoc[r] = s.id;
        }
    }
    if (tid == 0) {
        sarx_ktrack_header h = h0;
        const int made = table_full ? 0 : births;
        h.n_live = (uint32_t)(live + made);
        h.n_confirmed = (uint32_t)conf;
        h.next_id = h0.next_id + made;
        h.births_total = h0.births_total + (uint32_t)made;
        h.drops_total = h0.drops_total + (uint32_t)drops;
        h.t_last = a.f.t;
        if (table_full) {
            h.error = SARX_KTRACK_ERR_TABLE_OVERFLOW;
            h.error_frame = a.f.frame_index;
        } else {
            h.frames_done = h0.frames_done + 1;
        }
        *a.hdr = h;
    }
}

__global__ __launch_bounds__(256) void ktrack_init_kernel(sarx_ktrack_header* hdr, sarx_ktrack_slot* slots, int max_tracks) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < max_tracks) slots[t] = sarx_ktrack_slot{};
    if (t == 0) {
        sarx_ktrack_header h{};
        h.error_frame = -1;
        h.max_tracks = (uint32_t)max_tracks;
        *hdr = h;
    }
}

hipError_t launch_ktrack_init(sarx_ktrack_header* hdr, sarx_ktrack_slot* slots, int max_tracks, hipStream_t st) {
    ktrack_init_kernel<<<(max_tracks + 255) / 256, 256, 0, st>>>(hdr, slots, max_tracks);
    return hipGetLastError();
}

hipError_t launch_ktrack_step(const KtrackArgs& a, hipStream_t st) {
    const int n_tb = a.tp / KT_THREADS, n_rb = a.rp / KT_THREADS;
    ktrack_prepare_kernel<<<n_tb + n_rb, KT_THREADS, 0, st>>>(a, n_tb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ktrack_pair_kernel<<<n_tb + n_rb, KT_THREADS, 0, st>>>(a, n_tb);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    ktrack_update_kernel<<<n_tb, KT_THREADS, 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    ktrack_resolve_kernel<<<1, KT_RESOLVE_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace sarx
