// libsarx C ABI (include/sarx.h), the other focusers and the products: Range-Doppler plan, ATI / DPCA and the small product wrappers,
// echo synthesis, time-domain back-projection, noise and power statistics.
#include "api_ctx.h"
#include "csa_kernels.h"
#include "general.h"
#include "tdbp.h"

#include <cmath>
#include <cstdlib>
#include <mutex>
#include <set>
#include <string>
#include <vector>

using namespace sarx;

// the back-projection plans alive, for the entry points that refuse a destroyed one (tdbp_plan_usable, api_ctx.h)
static std::mutex g_plans_mu;
static std::set<const sarx_tdbp_plan*> g_plans;
void sarx::tdbp_plan_register(const sarx_tdbp_plan* p, bool alive) {
    std::lock_guard<std::mutex> lk(g_plans_mu);
    if (alive) g_plans.insert(p); else g_plans.erase(p);
}
bool sarx::tdbp_plan_live(const sarx_tdbp_plan* p) {
    std::lock_guard<std::mutex> lk(g_plans_mu);
    return p && g_plans.count(p) != 0;
}

extern "C" {

// ---- Range-Doppler focus ---------------------------------------------------------------
struct sarx_rda_plan {
    sarx_ctx* ctx = nullptr;
    Rda* r = nullptr;
    int n_r = 0, n_p = 0;
    float2* d_in = nullptr;
};

static int sarx_rda_plan_create_impl(sarx_ctx* c, int n_ranges, int n_pulses, const sarx_radar_params* prm, sarx_rda_plan** out) {
    NEED_CTX(c);
    if (!out || !prm) return fail(c, SARX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_ranges < 2 || n_pulses < 2 || n_ranges > 2 * TW_MAX || n_pulses > 2 * TW_MAX)
        return fail(c, SARX_ERR_UNSUPPORTED, "n_ranges=%d n_pulses=%d: sizes must be in [2, %d]", n_ranges, n_pulses, 2 * TW_MAX);
    if (!(prm->sample_rate_hz > 0) || !(prm->prf_hz > 0) || !(prm->platform_speed_mps > 0) || !(prm->wavelength_m > 0) ||
        !(prm->pulse_width_s > 0))
        return fail(c, SARX_ERR_INVALID, "radar parameters must be positive");
    std::string err;
    Rda* r = rda_create(n_ranges, n_pulses, prm, c->tw_all, err, c->cus);
    if (!r) return fail(c, SARX_ERR_UNSUPPORTED, "n_ranges=%d n_pulses=%d: %s", n_ranges, n_pulses, err.c_str());
    sarx_rda_plan* p = new sarx_rda_plan();
    p->ctx = c; p->r = r; p->n_r = n_ranges; p->n_p = n_pulses;
    hipError_t e = hipMalloc(&p->d_in, (size_t)n_ranges * n_pulses * sizeof(float2));
    if (e != hipSuccess) { rda_destroy(r); delete p; return fail(c, SARX_ERR_NOMEM, "hipMalloc: %s", hipGetErrorString(e)); }
    *out = p;
    return SARX_OK;
}
int sarx_rda_plan_create(sarx_ctx* c, int n_ranges, int n_pulses, const sarx_radar_params* prm, sarx_rda_plan** out) {
    return guarded(c, [&] { return sarx_rda_plan_create_impl(c, n_ranges, n_pulses, prm, out); });
}
int sarx_rda_plan_destroy(sarx_rda_plan* p) {
    if (!p) return SARX_OK;
    hipSetDevice(p->ctx->device);
    sync_all_lanes(p->ctx);
    rda_destroy(p->r);
    hipFree(p->d_in);
    delete p;
    return SARX_OK;
}
int sarx_rda_focus_host2(sarx_rda_plan* p, const void* phist, float* mag, void* pc, void* rd, void* rc, void* ac) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!phist || !mag) return fail(c, SARX_ERR_INVALID, "NULL host pointer");
    const size_t px = (size_t)p->n_r * p->n_p;
    HIPCHK(c, staged_copy(c, p->d_in, phist, px * sizeof(float2), true));
    HIPCHK(c, rda_focus(p->r, p->d_in, c->stream, nullptr, rc != nullptr, ac != nullptr));
    HIPCHK(c, staged_copy(c, mag, rda_mag(p->r), px * sizeof(float), false));
    void* outs[4] = {pc, rd, rc, ac};
    for (int i = 0; i < 4; ++i)
        if (outs[i]) HIPCHK(c, staged_copy(c, outs[i], rda_stage(p->r, i), px * sizeof(float2), false));
    return SARX_OK;
}
int sarx_rda_focus_host(sarx_rda_plan* p, const void* phist, float* mag, void* pc, void* rd, void* rc) {
    return sarx_rda_focus_host2(p, phist, mag, pc, rd, rc, nullptr);
}
int sarx_rda_focus_dev2(sarx_rda_plan* p, const void* d_phist, float* d_mag, void* d_pc, void* d_rd, void* d_rc, void* d_ac) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!d_phist || !d_mag) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    const size_t px = (size_t)p->n_r * p->n_p;
    HIPCHK(c, rda_focus(p->r, (const float2*)d_phist, c->stream, d_mag, d_rc != nullptr, d_ac != nullptr));   // magnitude written in place by the last launch
    void* outs[4] = {d_pc, d_rd, d_rc, d_ac};
    for (int i = 0; i < 4; ++i)
        if (outs[i]) HIPCHK(c, hipMemcpyAsync(outs[i], rda_stage(p->r, i), px * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
    return SARX_OK;
}
int sarx_rda_focus_dev(sarx_rda_plan* p, const void* d_phist, float* d_mag, void* d_pc, void* d_rd, void* d_rc) {
    return sarx_rda_focus_dev2(p, d_phist, d_mag, d_pc, d_rd, d_rc, nullptr);
}
int sarx_rda_axes(const sarx_rda_plan* p, double* range_centered, double* cross_range, double* doppler) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    rda_axes(p->r, range_centered, cross_range, doppler);
    return SARX_OK;
}

// ---- ATI / DPCA ------------------------------------------------------------------
static int ati_dpca_impl(sarx_ctx* c, const void* s1, const void* s2, size_t n, double cal_phase, const sarx_ati_outputs* o,
                         double* max_mag, double* sum2, const float* d_max, float mask_frac);
int sarx_ati_dpca_dev(sarx_ctx* c, const void* s1, const void* s2, size_t n, double cal_phase,
                      const sarx_ati_outputs* o, double* max_mag, double* sum2) {
    return ati_dpca_impl(c, s1, s2, n, cal_phase, o, max_mag, sum2, nullptr, 0.f);
}
int sarx_ati_dpca_masked_dev(sarx_ctx* c, const void* s1, const void* s2, size_t n, double cal_phase, const float* d_max,
                             float mask_frac, const sarx_ati_outputs* o) {
    NEED_CTX(c);
    if (!d_max) return fail(c, SARX_ERR_INVALID, "d_max is NULL (sarx_csa_plan_set_max_slot provides it)");
    return ati_dpca_impl(c, s1, s2, n, cal_phase, o, nullptr, nullptr, d_max, mask_frac);
}
static int ati_dpca_impl(sarx_ctx* c, const void* s1, const void* s2, size_t n, double cal_phase, const sarx_ati_outputs* o,
                         double* max_mag, double* sum2, const float* d_max, float mask_frac) {
    NEED_CTX(c);
    if (!s1 || !s2 || !o || !o->ati_phase || !o->slc1_mag || !o->dpca_mag) return fail(c, SARX_ERR_INVALID, "NULL required pointer");
    if (n == 0) { if (max_mag) *max_mag = 0; if (sum2) sum2[0] = sum2[1] = 0; return SARX_OK; }
    {   // the kernel moves 16 bytes per lane and plane
        const void* ptrs[] = {s1, s2, o->ati_phase, o->slc1_mag, o->dpca_mag, o->ati_interf, o->dpca_diff, o->slc2_mag,
                              o->slc1_phase, o->slc2_phase, o->dpca_phase};
        for (const void* q : ptrs)
            if (((uintptr_t)q) & 15) return fail(c, SARX_ERR_INVALID, "ATI/DPCA buffers must be 16-byte aligned");
    }
    AtiArgs a{};
    a.s1 = (const float2*)s1; a.s2 = (const float2*)s2; a.n = n;
    a.cal_c = (float)cos(cal_phase); a.cal_s = (float)sin(cal_phase);
    a.ati_phase = o->ati_phase; a.mag1 = o->slc1_mag; a.dpca_mag = o->dpca_mag;
    a.interf = (float2*)o->ati_interf; a.diff = (float2*)o->dpca_diff;
    a.mag2 = o->slc2_mag; a.ph1 = o->slc1_phase; a.ph2 = o->slc2_phase; a.dpca_phase = o->dpca_phase;
    a.part_max = c->ati_part_max_(); a.part_sum = c->ati_part_sum_();
    a.thr_max = d_max; a.mask_frac = mask_frac;
    // the two images are read for the last time here: nontemporal loads once they are too large to still be cached
    // (0.341 -> 0.329 ms at 8192^2); SARX_ATI_NT=0/1 overrides
    { static const int nt = [] { const char* e = getenv("SARX_ATI_NT"); return e ? atoi(e) : -1; }(); a.nt = nt < 0 ? n >= ((size_t)1 << 25) : nt != 0; }
    HIPCHK(c, launch_ati_dpca(a, c->stream));
    HIPCHK(c, launch_ati_finish(c->ati_part_max_(), c->ati_part_sum_(), ati_blocks(n), c->ati_out3_(), c->stream));
    if (max_mag || sum2) {
        double h[3];
        HIPCHK(c, hipMemcpyAsync(h, c->ati_out3_(), sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (max_mag) *max_mag = h[0];
        if (sum2) { sum2[0] = h[1]; sum2[1] = h[2]; }
    }
    return SARX_OK;
}

int sarx_ati_stats(sarx_ctx* c, double* max_mag, double* sum2) {
    NEED_CTX(c);
    double h[3];
    HIPCHK(c, hipMemcpyAsync(h, c->ati_out3_(), sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (max_mag) *max_mag = h[0];
    if (sum2) { sum2[0] = h[1]; sum2[1] = h[2]; }
    return SARX_OK;
}

int sarx_mask_phase_frac_dev(sarx_ctx* c, const float* phase, const float* mag, size_t n, float frac, float* out) {
    NEED_CTX(c);
    if (!phase || !mag || !out) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (n == 0) return SARX_OK;
    HIPCHK(c, launch_mask_phase_frac(phase, mag, n, frac, c->ati_out3_(), out, c->stream));
    return SARX_OK;
}

int sarx_magnitude_dev(sarx_ctx* c, const void* in, float* out, size_t n) {
    NEED_CTX(c);
    if (!in || !out) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (n) HIPCHK(c, launch_magnitude((const float2*)in, out, n, c->stream));
    return SARX_OK;
}

int sarx_max_abs_f32_dev(sarx_ctx* c, const float* x, size_t n, float* d_max) {
    NEED_CTX(c);
    if (!x || !d_max) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (n) HIPCHK(c, launch_max_abs_f32(x, n, d_max, c->stream));
    return SARX_OK;
}

int sarx_mask_phase_dev(sarx_ctx* c, const float* phase, const float* mag, size_t n, float thr, float* out) {
    NEED_CTX(c);
    if (!phase || !mag || !out) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (n == 0) return SARX_OK;
    HIPCHK(c, launch_mask_phase(phase, mag, n, thr, out, c->stream));
    return SARX_OK;
}

int sarx_corner_turn_dev(sarx_ctx* c, const void* in, void* out, int rows, int cols) {
    NEED_CTX(c);
    if (!in || !out || in == out || rows <= 0 || cols <= 0) return fail(c, SARX_ERR_INVALID, "bad corner-turn arguments");
    HIPCHK(c, launch_corner_turn((const float2*)in, (float2*)out, rows, cols, c->stream));
    return SARX_OK;
}

int sarx_multilook_dev(sarx_ctx* c, const void* in, float* out, int rows, int cols, int looks) {
    NEED_CTX(c);
    if (!in || !out) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (looks < 1 || looks > 512 || (looks & (looks - 1)) || rows % looks || cols % looks || (cols & 1))
        return fail(c, SARX_ERR_UNSUPPORTED, "looks=%d must be a power of two <= 512 dividing rows=%d and cols=%d", looks, rows, cols);
    HIPCHK(c, launch_multilook((const float2*)in, out, rows, cols, looks, c->stream));
    return SARX_OK;
}

int sarx_echo_synth_dev(sarx_ctx* c, const double* tau_pb, const float* amp, const double* t_fast, int n_pulses,
                        int n_targets, int n_samples, double kr, double t_p, void* raw, int accumulate) {
    NEED_CTX(c);
    if (!tau_pb || !amp || !t_fast || !raw) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (n_pulses <= 0 || n_targets <= 0 || n_samples <= 0 || n_pulses > 65535)
        return fail(c, SARX_ERR_INVALID, "echo sizes must be positive (n_pulses <= 65535 per call)");
    EchoArgs a{};
    a.tau_pb = (const double2*)tau_pb; a.amp = amp; a.t_fast = t_fast; a.out = (float2*)raw;
    a.kr = kr; a.t_p = t_p; a.u_off = 0.5 * t_p; a.n_pulses = n_pulses; a.n_targets = n_targets; a.n_samples = n_samples;
    a.accumulate = accumulate != 0;
    HIPCHK(c, launch_echo_synth(a, c->stream));
    return SARX_OK;
}
int sarx_echo_geometry_dev(sarx_ctx* c, int model, int n_pulses, int n_targets, const double* tgt_pos, const double* tgt_vel,
                           const double* t_pulse, const double* tx_pos, const double* aux, const double* rcs, double c_light,
                           double fc, double l_ant, double wavelength, double* tau_pb, float* amp_pt) {
    NEED_CTX(c);
    if (model < 0 || model > 2) return fail(c, SARX_ERR_INVALID, "echo model must be 0, 1 or 2");
    if (n_pulses <= 0 || n_targets <= 0 || n_pulses > 65535) return fail(c, SARX_ERR_INVALID, "echo sizes must be positive (n_pulses <= 65535 per call)");
    if (!tgt_pos || !tx_pos || !tau_pb) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (model != 0 && (!tgt_vel || !t_pulse || !aux)) return fail(c, SARX_ERR_INVALID, "models 1 and 2 need target velocity, pulse times and aux");
    if (model == 0 && tgt_vel && !t_pulse) return fail(c, SARX_ERR_INVALID, "moving targets need the pulse times");
    if (model == 2 && (!rcs || !amp_pt || !(wavelength > 0))) return fail(c, SARX_ERR_INVALID, "model 2 needs rcs, amp_pt and the wavelength");
    if (!(c_light > 0) || !(fc > 0)) return fail(c, SARX_ERR_INVALID, "C and FC must be positive");
    EchoGeoArgs a{};
    a.model = model; a.n_pulses = n_pulses; a.n_targets = n_targets;
    a.tgt_pos = tgt_pos; a.tgt_vel = tgt_vel; a.t_pulse = t_pulse; a.tx_pos = tx_pos; a.aux = aux; a.rcs = rcs;
    a.c = c_light; a.fc = fc; a.l_ant = l_ant; a.lambda = wavelength;
    a.tau_pb = (double2*)tau_pb; a.amp_pt = amp_pt;
    HIPCHK(c, launch_echo_geometry(a, c->stream));
    return SARX_OK;
}
int sarx_echo_spotlight_dev(sarx_ctx* c, const double* tau_pb, const float* amp_pt, const double* t_fast, int n_pulses,
                            int n_targets, int n_samples, double kr, double t_p, void* raw) {
    NEED_CTX(c);
    if (!tau_pb || !amp_pt || !t_fast || !raw) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (n_pulses <= 0 || n_targets <= 0 || n_samples <= 0 || n_pulses > 65535)
        return fail(c, SARX_ERR_INVALID, "echo sizes must be positive (n_pulses <= 65535 per call)");
    EchoArgs a{};
    a.tau_pb = (const double2*)tau_pb; a.amp_pt = amp_pt; a.t_fast = t_fast; a.out = (float2*)raw;
    a.kr = kr; a.t_p = t_p; a.u_off = 0.0; a.n_pulses = n_pulses; a.n_targets = n_targets; a.n_samples = n_samples;
    HIPCHK(c, launch_echo_synth(a, c->stream));
    return SARX_OK;
}

// ---- time-domain back-projection ---------------------------------------------------------
// struct sarx_tdbp_plan: api_ctx.h (api_tdbp_search.hip and api_tdbp_pair.hip take plans too); the list of live ones: the head of this file

static int sarx_tdbp_plan_create_impl(sarx_ctx* c, int n_pulses, int num_samples, int nx, int ny, const sarx_tdbp_params* k,
                          sarx_tdbp_plan** out) {
    NEED_CTX(c);
    if (!out || !k) return fail(c, SARX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_pulses < 1 || num_samples < 2 || nx < 1 || ny < 1 || nx > 65536 || ny > 65536)
        return fail(c, SARX_ERR_INVALID, "n_pulses=%d num_samples=%d nx=%d ny=%d: sizes must be positive", n_pulses, num_samples, nx, ny);
    if (!(k->c > 0) || !(k->fc > 0) || !(k->fs > 0) || !(k->t_p > 0) || !(k->k_rate != 0))
        return fail(c, SARX_ERR_INVALID, "TDBP constants must be positive");
    std::string err;
    Tdbp* t = tdbp_create(n_pulses, num_samples, nx, ny, k, c->tw_all, err);
    if (!t) return fail(c, SARX_ERR_UNSUPPORTED, "tdbp plan: %s", err.c_str());
    sarx_tdbp_plan* p = new sarx_tdbp_plan();
    p->ctx = c; p->t = t; p->n_p = n_pulses; p->n_s = num_samples; p->nx = nx; p->ny = ny;
    tdbp_plan_register(p, true);
    *out = p;
    return SARX_OK;
}
int sarx_tdbp_plan_create(sarx_ctx* c, int n_pulses, int num_samples, int nx, int ny, const sarx_tdbp_params* k,
                          sarx_tdbp_plan** out) {
    return guarded(c, [&] { return sarx_tdbp_plan_create_impl(c, n_pulses, num_samples, nx, ny, k, out); });
}
int sarx_tdbp_plan_destroy(sarx_tdbp_plan* p) {
    if (!p) return SARX_OK;
    tdbp_plan_register(p, false);
    hipSetDevice(p->ctx->device);
    sync_all_lanes(p->ctx);
    tdbp_destroy(p->t);
    hipFree(p->d_raw);
    delete p;
    return SARX_OK;
}
int sarx_tdbp_focus_dev(sarx_tdbp_plan* p, const void* d_raw, const double* pos, const double* vel, const double* t_pulses,
                        double t_start, const double* vel_focus, double scene_size, void* d_image) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!d_raw || !pos || !vel || !t_pulses || !vel_focus || !d_image) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (!(scene_size > 0)) return fail(c, SARX_ERR_INVALID, "scene_size must be positive");
    HIPCHK(c, tdbp_focus(p->t, (const float2*)d_raw, pos, vel, t_pulses, t_start, vel_focus, scene_size, false, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_image, tdbp_image(p->t), (size_t)p->nx * p->ny * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
    return SARX_OK;
}
int sarx_tdbp_last_window(const sarx_tdbp_plan* p, int* lo, int* hi) {
    if (!p || !lo || !hi) return fail(nullptr, SARX_ERR_INVALID, "NULL argument");
    tdbp_window(p->t, lo, hi);
    return SARX_OK;
}
int sarx_tdbp_focus_host(sarx_tdbp_plan* p, const void* raw, const double* pos, const double* vel, const double* t_pulses,
                         double t_start, const double* vel_focus, double scene_size, void* image, void* range_compressed) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!raw || !pos || !vel || !t_pulses || !vel_focus || !image) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (!(scene_size > 0)) return fail(c, SARX_ERR_INVALID, "scene_size must be positive");
    const size_t n = (size_t)p->n_p * p->n_s;
    if (const int rc = tdbp_plan_raw(c, p)) return rc;
    HIPCHK(c, staged_copy(c, p->d_raw, raw, n * sizeof(float2), true));
    HIPCHK(c, tdbp_focus(p->t, p->d_raw, pos, vel, t_pulses, t_start, vel_focus, scene_size, range_compressed != nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(image, tdbp_image(p->t), (size_t)p->nx * p->ny * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    if (range_compressed) HIPCHK(c, hipMemcpyAsync(range_compressed, tdbp_rc(p->t), n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SARX_OK;
}

int sarx_fill_noise_c64(sarx_ctx* c, void* buf, size_t n, uint64_t seed) {
    NEED_CTX(c);
    if (!buf) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (n) HIPCHK(c, launch_fill_noise((float2*)buf, n, seed, c->stream));
    return SARX_OK;
}

int sarx_add_ocean_noise_dev(sarx_ctx* c, void* buf, size_t n, double noise_std, double clutter_power, double k_nu,
                             uint64_t seed) {
    NEED_CTX(c);
    if (!buf) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (!(noise_std >= 0) || !(clutter_power >= 0) || (clutter_power > 0 && !(k_nu > 0)))
        return fail(c, SARX_ERR_INVALID, "noise_std, clutter_power must be >= 0 and k_nu > 0");
    if (n) HIPCHK(c, launch_ocean_noise((float2*)buf, n, (float)noise_std, (float)clutter_power, (float)k_nu, seed, c->stream));
    return SARX_OK;
}
int sarx_add_ocean_noise_rel_dev(sarx_ctx* c, void* buf, size_t n, int ref_is_max, double snr_lin, double scr_lin, double k_nu,
                                 uint64_t seed) {
    NEED_CTX(c);
    if (!buf || !n) return fail(c, SARX_ERR_INVALID, "empty buffer");
    if (!(snr_lin > 0) || !(scr_lin >= 0) || (scr_lin > 0 && !(k_nu > 0)))
        return fail(c, SARX_ERR_INVALID, "snr_lin must be > 0, scr_lin >= 0 (0 = thermal noise only) and k_nu > 0");
    double* d_part = c->power_part_all + (size_t)c->cur_lane * sarx_ctx::POWER_STRIDE;
    float* d_levels = reinterpret_cast<float*>(d_part + 2048);
    HIPCHK(c, launch_power_stats((const float2*)buf, n, d_part, 1024, c->stream));
    HIPCHK(c, launch_noise_levels(d_part, 1024, n, ref_is_max != 0, snr_lin, scr_lin, d_levels, c->stream));
    HIPCHK(c, launch_ocean_noise((float2*)buf, n, 0.f, 0.f, (float)k_nu, seed, c->stream, d_levels));
    return SARX_OK;
}
static int sarx_power_stats_dev_impl(sarx_ctx* c, const void* buf, size_t n, double* max_abs2, double* mean_abs2) {
    NEED_CTX(c);
    if (!buf || !n) return fail(c, SARX_ERR_INVALID, "empty buffer");
    const int blocks = 1024;
    double* d_part = c->power_part_all + (size_t)c->cur_lane * sarx_ctx::POWER_STRIDE;
    hipError_t e = launch_power_stats((const float2*)buf, n, d_part, blocks, c->stream);
    std::vector<double> part(2 * blocks);
    if (e == hipSuccess) e = hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIPCHK(c, e);
    double sum = 0.0, mx = 0.0;
    for (int b = 0; b < blocks; ++b) { sum += part[2 * b]; if (part[2 * b + 1] > mx) mx = part[2 * b + 1]; }
    if (max_abs2) *max_abs2 = mx;
    if (mean_abs2) *mean_abs2 = sum / (double)n;
    return SARX_OK;
}
int sarx_power_stats_dev(sarx_ctx* c, const void* buf, size_t n, double* max_abs2, double* mean_abs2) {
    return guarded(c, [&] { return sarx_power_stats_dev_impl(c, buf, n, max_abs2, mean_abs2); });
}

}  // extern "C"
