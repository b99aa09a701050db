// Two-receiver back-projection: both receive channels of the two-receiver echo model
// (sar_ati_dcpa_sim_csa.py:113-178) imaged onto one ground grid in one enqueue.  It is the N = 2 case of the receiver stack of
// tdbp_multi.hip - the steps, the kernels and the scratch's functions are stated there - run on an instance of its own (t->pair), so that a
// plan that images pairs alone holds two channels' memory and the pair's route answers for the pair's calls.
//
// Here: what the geometry of a receiver displaced along the track asks of the host, for the stack, the pair and the pair's search
// (tdbp_pair_search.hip) alike - the bounds that choose the sample window and the kernel (tdbp_pair_bounds) and the per-pulse table
// (tdbp_pair_table) - and the pair's entry points, each a few lines on the stack's routine.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "tdbp_plan.h"

namespace sarx {

static_assert(sizeof(sarx_tdbp_pair_params) == 40, "sarx_tdbp_pair_params is 40 bytes");

// Sample window [lo, hi) that any channel can touch over the pulses [u0, u1), whether the series of tdbp_pair_pixel holds, and
// whether the receivers' part of the tile expansion does (the d_tx part is tdbp_tile_ok's).  om: the largest |offset| of the channels.
// d_tx lies in moved_rect_range (tdbp.hip); a receiver is at most om from the transmitter, so |d_rx - d_tx| <= om (triangle inequality)
// and |e| = |d_rx^2 / d_tx^2 - 1| <= 2 om / d_tx + (om / d_tx)^2: one window, one series test and one tile test hold for every channel.
void tdbp_pair_bounds(const Tdbp* t, const std::vector<PulseGeo>& geo, int u0, int u1, const double* vf, double t_start, double scene_size,
                      double om, double chirp_centre, int* lo, int* hi, bool* series, bool* tile) {
    const double c = t->k.c, fs = t->k.fs, h = scene_size / 2;
    double imin = 1e300, imax = -1e300;
    *series = true;
    // the remainder of d_tx - d_rx about a tile's reference pixel (tdbp_pixel.hpp): |q|^2 |off| / (sqrt(3) (d_min - |off|)^2), q the
    // tile's reach (tdbp_tile_reach), as tdbp_tile_ok takes it
    const double qm = tdbp_tile_reach(t, scene_size);
    *tile = qm >= 0.0;
    for (int p = u0; p < u1; ++p) {
        double dmin, dmax;
        moved_rect_range(geo[p], vf, h, &dmin, &dmax);
        const double a = ((2.0 * dmin - om) / c - t_start + chirp_centre) * fs;
        const double b = ((2.0 * dmax + om) / c - t_start + chirp_centre) * fs;
        if (a < imin) imin = a;
        if (b > imax) imax = b;
        const double e = 2.0 * om / dmin + (om / dmin) * (om / dmin);
        if (!(dmin > 0.0) || !(7.0 / 256.0 * e * e * e * e * e * dmax < 1e-9)) *series = false;
        if (!(dmin > om) || !(qm * qm * om / (sqrt(3.0) * (dmin - om) * (dmin - om)) < 1e-9)) *tile = false;
    }
    tdbp_clamp_window(imin, imax, t->n_s, lo, hi);
}

void tdbp_pair_table(PairGeo* h_geo, const std::vector<PulseGeo>& geo, const double* vel, int n_p) {
    for (int p = 0; p < n_p; ++p) {
        PairGeo& g = h_geo[p];
        const double vx = vel[3 * p], vy = vel[3 * p + 1], vz = vel[3 * p + 2];
        const double inv = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
        g.px = geo[p].px; g.py = geo[p].py; g.pz = geo[p].pz;
        g.ux = vx * inv; g.uy = vy * inv; g.uz = vz * inv;
        g.dt = geo[p].dt; g.pad = 0.0;
    }
}

hipError_t tdbp_pair_rc1(Tdbp* t, cf** rc1) {
    TdbpRx* s = nullptr;
    TCK(tdbp_rx_scratch(t, t->pair, 2, 2, &s));
    *rc1 = s->rc[0];
    return hipSuccess;
}

hipError_t tdbp_pair(Tdbp* t, const float2* raw0, const float2* raw1, const double* pos, const double* vel, const double* t_pulses,
                     double t_start, const double* vel_focus, double scene_size, const sarx_tdbp_pair_params* prm, int chunks,
                     double2* d_img128, float2* d_img64, hipStream_t st) {
    const float2* const raw[2] = {raw0, raw1};
    const sarx_tdbp_multi_params m = tdbp_pair_as_multi(*prm);
    return tdbp_rx(t, t->pair, 2, raw, pos, vel, t_pulses, t_start, vel_focus, scene_size, &m, chunks, d_img128, d_img64, st);
}

int tdbp_pair_route(const Tdbp* t) { return t->pair ? t->pair->route : -1; }

hipError_t tdbp_pair_staging(Tdbp* t, float2** d_raw1, double2** d_img128, float2** d_img64) {
    return tdbp_rx_staging(t, t->pair, 2, 2, d_raw1, d_img128, d_img64);
}

}  // namespace sarx
