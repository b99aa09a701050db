// Ground relocation of GMTI reports (include/sarx_relocate.h): two launches.
//   solve : one lane per report of the input slot (the count read from its header on the device) writes the report's record and a
//           sort key: (io, jo, r) packed into one word, io << 34 | jo << 14 | r (20 + 20 + 14 bits: the order of (io out_nx + jo, r)
//           in a single comparison and without a division to undo it), or KEY_NONE for a report that is not kept.  Per report two
//           square roots (R, sqrt(h2)) and four divisions (al, the two pixel coordinates, 1 / R), two more for a velocity; what
//           depends on vel_ref alone (sqrt(s2), a) is formed once on the host.
//   slot  : a kept report's place in the output slot is the number of keys below its own, counted against the keys staged through
//           LDS 256 at a time as gmti_refine_kernel does (a stage is always 256 keys, padded with KEY_NONE, which is below nothing:
//           the count loop has a fixed length and unrolls, so its LDS reads overlap); workgroup 0 counts the kept keys on the way and
//           closes the header.  The compaction ranks of gmti_dev.hpp (thread order) do not serve a sort by pixel; its slot view and
//           slot_close do.
// Each record, key and output report has one writer and no sum crosses lanes: the same bits on every run.
#include "relocate.h"

#include <climits>

#include "gmti_dev.hpp"

namespace sarx {

static_assert(sizeof(sarx_relocate_params) == 128, "sarx_relocate_params is 128 bytes");
static_assert(sizeof(sarx_relocate_record) == 64, "sarx_relocate_record is 64 bytes");
static_assert(sizeof(sarx_gmti_report) == 48, "a report is copied as 48 bytes without padding");

static constexpr int RELOCATE_THREADS = 256;
static constexpr long long KEY_NONE = LLONG_MAX;
static constexpr int KEY_R_BITS = 14, KEY_PIXEL_BITS = 20;
static_assert(SARX_TDBP_MULTI_MAX_DETECTIONS <= 1 << KEY_R_BITS && SARX_TDBP_MULTI_MAX_DIM <= 1 << KEY_PIXEL_BITS,
              "the sort key holds io, jo and r in 20 + 20 + 14 bits");

__global__ __launch_bounds__(RELOCATE_THREADS) void relocate_solve_kernel(RelocateArgs a, double vs, double ax, double ay) {
    const SlotView s = slot_view(a.in, a.p.max_detections);
    const unsigned r = blockIdx.x * (unsigned)RELOCATE_THREADS + threadIdx.x;
    sarx_relocate_record out{};
    if (s.unusable) {                                                  // never a truncated answer
        out.status = SARX_RELOCATE_OVERFLOW;
        if (r == 0) a.rec[0] = out;
        return;
    }
    if (r >= s.count) return;
    out.rank = -1;
    long long key = KEY_NONE;
    const double v_los = *(const double*)(a.v_los + (size_t)r * a.v_los_stride);
    const bool invalid = a.valid && *(const uint32_t*)(a.valid + (size_t)r * a.valid_stride) != 0u;
    const sarx_relocate_params& p = a.p;
    const double qx = p.in_x0 + (double)s.rep[r].j * p.in_dx, qy = p.in_y0 + (double)s.rep[r].i * p.in_dy;
    const double wx = qx - p.pos_ref[0], wy = qy - p.pos_ref[1], h = -p.pos_ref[2];
    const double rho2 = wx * wx + wy * wy;
    const double R = sqrt(rho2 + h * h);
    const double al = (wx * p.vel_ref[0] + wy * p.vel_ref[1] + v_los * R) / vs;
    const double h2 = rho2 - al * al;
    if (invalid || !isfinite(v_los)) {
        out.status = SARX_RELOCATE_NO_SPEED;
    } else if (vs == 0.0 || !(rho2 > 0.0) || !(h2 >= 0.0)) {
        out.status = SARX_RELOCATE_NO_SOLUTION;
    } else {
        const double nx = -ay, ny = ax;
        const double across = wx * nx + wy * ny >= 0.0 ? sqrt(h2) : -sqrt(h2);
        const double ux = al * ax + across * nx, uy = al * ay + across * ny;      // (g - P) on the ground
        out.x = p.pos_ref[0] + ux;
        out.y = p.pos_ref[1] + uy;
        out.shift_x = out.x - qx;
        out.shift_y = out.y - qy;
        const double v_along = a.v_along ? *(const double*)(a.v_along + (size_t)r * a.v_along_stride) : NAN;
        if (isfinite(v_along)) {
            const double ex = ux / R, ey = uy / R;
            const double det = ex * ay - ey * ax;
            const double vx = (v_los * ay - ey * v_along) / det, vy = (ex * v_along - ax * v_los) / det;
            if (det != 0.0 && isfinite(vx) && isfinite(vy)) {
                out.vx = vx;
                out.vy = vy;
                out.flags = SARX_RELOCATE_HAS_VELOCITY;
            }
        }
        // compared as fp64: a position far off the grid has no int
        const double fj = floor((out.x - p.out_x0) / p.out_dx + 0.5), fi = floor((out.y - p.out_y0) / p.out_dy + 0.5);
        if (fj >= 0.0 && fj < (double)p.out_nx && fi >= 0.0 && fi < (double)p.out_ny) {
            out.status = SARX_RELOCATE_OK;
            key = ((((long long)fi << KEY_PIXEL_BITS) | (long long)fj) << KEY_R_BITS) | (long long)r;
        } else {
            out.status = SARX_RELOCATE_OFF_GRID;
        }
    }
    a.rec[r] = out;
    a.keys[r] = key;
}

__global__ __launch_bounds__(RELOCATE_THREADS) void relocate_slot_kernel(RelocateArgs a) {
    __shared__ long long keys[RELOCATE_THREADS];
    const SlotView s = slot_view(a.in, a.p.max_detections);
    if (s.unusable) {
        if (blockIdx.x == 0 && threadIdx.x == 0) slot_close(a.out, s.count, true);
        return;
    }
    const int n = (int)s.count;
    if (blockIdx.x != 0 && (int)(blockIdx.x * RELOCATE_THREADS) >= n) return;     // workgroup-uniform; workgroup 0 closes the header
    const int t = blockIdx.x * RELOCATE_THREADS + threadIdx.x;
    const long long mine = t < n ? a.keys[t] : KEY_NONE;
    int rank = 0, kept = 0;
    for (int b = 0; b < n; b += RELOCATE_THREADS) {
        __syncthreads();
        const int k = b + threadIdx.x;
        const long long staged = k < n ? a.keys[k] : KEY_NONE;
        keys[threadIdx.x] = staged;
        kept += __syncthreads_count(staged != KEY_NONE);
#pragma unroll 16
        for (int q = 0; q < RELOCATE_THREADS; ++q) rank += keys[q] < mine;
    }
    if (t == 0) slot_close(a.out, (uint32_t)kept, false);
    if (mine == KEY_NONE) return;
    sarx_gmti_report rep = s.rep[t];
    rep.i = (int32_t)(mine >> (KEY_PIXEL_BITS + KEY_R_BITS));
    rep.j = (int32_t)((mine >> KEY_R_BITS) & ((1LL << KEY_PIXEL_BITS) - 1));
    slot_reports(a.out)[rank] = rep;
    a.rec[t].rank = rank;
}

hipError_t launch_relocate(const RelocateArgs& a, hipStream_t st) {
    const double vs = sqrt(a.p.vel_ref[0] * a.p.vel_ref[0] + a.p.vel_ref[1] * a.p.vel_ref[1]);
    const double ax = vs > 0.0 ? a.p.vel_ref[0] / vs : 0.0, ay = vs > 0.0 ? a.p.vel_ref[1] / vs : 0.0;
    const dim3 grid((unsigned)((a.p.max_detections + RELOCATE_THREADS - 1) / RELOCATE_THREADS));
    hipLaunchKernelGGL(relocate_solve_kernel, grid, dim3(RELOCATE_THREADS), 0, st, a, vs, ax, ay);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(relocate_slot_kernel, grid, dim3(RELOCATE_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sarx
