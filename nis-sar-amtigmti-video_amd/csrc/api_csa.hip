// libsarx C ABI (include/sarx.h), chirp-scaling focus: the CSA plan (fp64 migration tables, scratch), pass orchestration, slab mode and
// the two-deep host pipeline.
#include "api_ctx.h"
#include "csa_kernels.h"
#include "general.h"

#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

using namespace sarx;

struct sarx_plan {
    sarx_ctx* ctx = nullptr;
    int n_az = 0, n_rg = 0;
    unsigned flags = 0;
    sarx_radar_params p{};
    int az_s = 0;          // four-step split: n_az = (n_az/az_s) * az_s; az_s == n_az means single step
    int az_w = 32;         // azimuth tile width (range samples)
    int az_w_alone = 0;    // > 0: width of the plain azimuth launches while the focus has the chip to itself (no CU share set): 64 columns =
                           // 512-byte row segments at 16384^2, 1.57-1.58 against 1.62-1.66 ms per two-launch transform; with frames in flight
                           // the 64 KiB tiles share CUs worse with the other lane's range launch (4.03-4.09 against 3.99-4.00 ms per frame),
                           // at 8192^2 and below nothing changes (profiles/r05_p_az_tile_width.log)
    int az_impl = 1;       // SARX_AZ_IMPL: 1 = the 128-point steps of n_az = 16384 (TWIDDLE / PHI1 / SCALE epilogues) run as wave-private
                           // tiles (az_wave.hip) whatever the tile width, CU share or slab mode; 0 = az_tile_kernel everywhere
    int az_wpb = 4;        // SARX_AZ_WAVES: waves (independent tiles) per workgroup of those launches, 1 or 4 (4: 0.73-0.75 against
                           // 0.83-0.84 ms per step alone at 16384^2, profiles/az_wave_steps.jsonl)
    int look = 0;          // > 0: the last azimuth launch also writes row-wise |x|^2 partials and a finish launch turns them into look_slot
    float* look_slot = nullptr;   // caller's [n_az/look x n_rg/look] fp32 slot (device)
    float* look_part = nullptr;   // [n_az x n_rg/look], owned by the plan
    // sarx_csa_plan_set_ati: the last azimuth launch emits the ATI / DPCA products of (ati_s1, the image being written)
    const float2* ati_s1 = nullptr; const float* ati_thr = nullptr; float ati_frac = 0.f; double ati_cal = 0.0;
    float *ati_phase = nullptr, *ati_m1 = nullptr, *ati_dm = nullptr; int ati_keep_image = 0;
    double2* ati_part = nullptr; int ati_nparts = 0;
    int ati_w = 32;                    // tile width of that launch: 64 columns where n_rg allows (256-byte row segments of the fp32 planes)
    float* max_slot = nullptr;         // sarx_csa_plan_set_max_slot: device float that receives max |image| of every focus
    bool az_nt = false;    // azimuth tile launches use nontemporal accesses (images >= 512 MiB; SARX_AZ_NT=0/1 overrides)
    int slab_tiles = 0;    // > 0: slab mode of sarx_csa_focus_dev with this many azimuth tiles per group (SARX_SLAB_MIB)
    double2 *c1 = nullptr, *c2 = nullptr, *c3 = nullptr;
    float2* buf_b = nullptr;           // scratch image
    float2* buf_a = nullptr;           // second scratch (RG_MAJOR only)
    float2 *h_in = nullptr, *h_out = nullptr;   // device staging for the *_host entry point
    // sarx_csa_focus_host_begin / _end: PIPE frames in flight between upload, focus and download
    static constexpr int PIPE = 2;
    float2 *pipe_in[PIPE] = {}, *pipe_out[PIPE] = {};
    int pipe_dl[PIPE] = {-1, -1};           // ctx download slot of the frame in pipeline slot i, -1 = free
    void* pipe_host[PIPE] = {};             // pageable destination of slot i (downloaded by _end), NULL when the DMA already targets it
    int pipe_next = 0;
    uint64_t bytes = 0;
    int mark_start = -1, mark_stop = -1;   // ctx event slots recorded around the range pass(es)
    unsigned long long* stamp = nullptr;   // sarx_csa_plan_stamp_range: {min start, max end} of the fused range launch (s_memrealtime ticks)
    GeneralCsa* gen = nullptr;             // chirp-z path for sizes that are not powers of two in [16, 16384]
};

static bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
static int ilog2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

extern "C" {

// ---- CSA plan -----------------------------------------------------------------
static int sarx_csa_plan_create_impl(sarx_ctx* c, int n_az, int n_rg, const sarx_radar_params* prm, unsigned flags, sarx_plan** out) {
    NEED_CTX(c);
    if (!out || !prm) return fail(c, SARX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_az < 2 || n_rg < 2 || n_az > 2 * TW_MAX || n_rg > 2 * TW_MAX)
        return fail(c, SARX_ERR_UNSUPPORTED, "n_az=%d n_rg=%d: sizes must be in [2, %d]", n_az, n_rg, 2 * TW_MAX);
    if (flags & ~(SARX_OUT_RG_MAJOR | SARX_FUSE_RANGE)) return fail(c, SARX_ERR_INVALID, "unknown plan flags 0x%x", flags);
    const bool general = !is_pow2(n_az) || !is_pow2(n_rg) || n_az < 16 || n_rg < 16 || n_az > TW_MAX || n_rg > TW_MAX;
    if (!(prm->sample_rate_hz > 0) || !(prm->prf_hz > 0) || !(prm->platform_speed_mps > 0) ||
        !(prm->wavelength_m > 0) || prm->chirp_rate_hz_s == 0.0)
        return fail(c, SARX_ERR_INVALID, "radar parameters must be positive (chirp rate non-zero)");
    sarx_plan* p = new sarx_plan();
    p->ctx = c; p->n_az = n_az; p->n_rg = n_rg; p->flags = flags; p->p = *prm;
    if (general) {       // any other size: chirp-z transforms over the power-of-two kernels (general.hip)
        std::string err;
        p->gen = general_csa_create(n_az, n_rg, prm, c->tw_all, err, true, c->cus);
        if (!p->gen) { delete p; return fail(c, SARX_ERR_UNSUPPORTED, "n_az=%d n_rg=%d: %s", n_az, n_rg, err.c_str()); }
        p->bytes = general_csa_bytes(p->gen);
        if (flags & SARX_OUT_RG_MAJOR) {
            hipError_t e2 = hipMalloc(&p->buf_a, (size_t)n_az * n_rg * sizeof(float2));
            if (e2 != hipSuccess) { int rc = fail(c, SARX_ERR_NOMEM, "hipMalloc: %s", hipGetErrorString(e2)); sarx_csa_plan_destroy(p); return rc; }
            p->bytes += (size_t)n_az * n_rg * sizeof(float2);
        }
        *out = p;
        return SARX_OK;
    }
    p->az_s = (n_az <= 128) ? n_az : (1 << (ilog2(n_az) / 2));
    p->az_w = (n_rg % 32 == 0) ? 32 : 16;
    p->az_nt = (size_t)n_az * n_rg * sizeof(float2) >= ((size_t)1 << 29);     // 8192^2 and up (measured: +2 % / +3.8 % at 8192^2 / 16384^2, -3 % at 4096^2)
    if (const char* e = getenv("SARX_AZ_NT")) p->az_nt = atoi(e) != 0;
    if (const char* e = getenv("SARX_SLAB_MIB")) {     // rows of one group of tiles, in MiB (0 = off)
        const double mib = atof(e);
        const double tile_mib = (double)p->az_s * n_rg * sizeof(float2) / (1024.0 * 1024.0);
        if (mib > 0 && p->az_s != n_az) {
            int q = (int)(mib / tile_mib);
            if (q < 1) q = 1;
            if (q > n_az / p->az_s) q = n_az / p->az_s;
            p->slab_tiles = q;
        }
    }
    if (const char* e = getenv("SARX_AZ_W")) { const int w = atoi(e); if ((w == 16 || w == 32 || w == 64) && n_rg % w == 0) p->az_w = w; }
    else if (n_rg % 64 == 0 && (size_t)n_az * n_rg * sizeof(float2) >= ((size_t)1 << 31)) p->az_w_alone = 64;
    if (const char* e = getenv("SARX_AZ_IMPL")) p->az_impl = atoi(e) != 0;
    if (const char* e = getenv("SARX_AZ_WAVES")) { const int w = atoi(e); if (w == 1 || w == 4) p->az_wpb = w; }

    // migration factors, natural fftfreq order (sar_ati_dcpa_sim_csa.py:225,244-249,262)
    const double lam = prm->wavelength_m, Kr = prm->chirp_rate_hz_s, Vr = prm->platform_speed_mps, Rref = prm->range_ref_m;
    const double fa_step = 1.0 / ((double)n_az * (1.0 / prm->prf_hz));
    std::vector<double2> c1(n_az), c2(n_az), c3(n_az);
    for (int i = 0; i < n_az; ++i) {
        const int ks = (i < n_az / 2) ? i : i - n_az;
        const double fa = (double)ks * fa_step;
        const double u = lam * fa / (2.0 * Vr);
        double arg = 1.0 - u * u;
        if (arg < 0) arg = 1e-9;                           // :246 sets, does not clamp to 0
        const double D = sqrt(arg);
        const double Cs = 1.0 / D - 1.0;
        const double tau_ref = 2.0 * Rref / (C_LIGHT * D);
        c1[i] = make_double2(-0.5 * Kr * Cs, tau_ref);
        c2[i] = make_double2(0.5 / (Kr * (1.0 + Cs)), 2.0 * Rref * Cs / C_LIGHT);
        c3[i] = make_double2(C_LIGHT * D / lam, -0.5 * Kr * Cs * (1.0 + Cs));
    }
    const size_t tb = (size_t)n_az * sizeof(double2), img = (size_t)n_az * n_rg * sizeof(float2);
    auto bail = [&](hipError_t e, const char* what) {
        int rc = fail(c, e == hipErrorOutOfMemory ? SARX_ERR_NOMEM : SARX_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
        sarx_csa_plan_destroy(p);
        return rc;
    };
    hipError_t e;
    if ((e = hipMalloc(&p->c1, tb)) != hipSuccess) return bail(e, "hipMalloc c1");
    if ((e = hipMalloc(&p->c2, tb)) != hipSuccess) return bail(e, "hipMalloc c2");
    if ((e = hipMalloc(&p->c3, tb)) != hipSuccess) return bail(e, "hipMalloc c3");
    if ((e = hipMemcpy(p->c1, c1.data(), tb, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "upload c1");
    if ((e = hipMemcpy(p->c2, c2.data(), tb, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "upload c2");
    if ((e = hipMemcpy(p->c3, c3.data(), tb, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "upload c3");
    if ((e = hipMalloc(&p->buf_b, img)) != hipSuccess) return bail(e, "hipMalloc scratch image");
    p->bytes = 3 * tb + img;
    if (flags & SARX_OUT_RG_MAJOR) {
        if ((e = hipMalloc(&p->buf_a, img)) != hipSuccess) return bail(e, "hipMalloc second scratch image");
        p->bytes += img;
    }
    *out = p;
    return SARX_OK;
}
int sarx_csa_plan_create(sarx_ctx* c, int n_az, int n_rg, const sarx_radar_params* prm, unsigned flags, sarx_plan** out) {
    return guarded(c, [&] { return sarx_csa_plan_create_impl(c, n_az, n_rg, prm, flags, out); });
}

int sarx_csa_plan_destroy(sarx_plan* p) {
    if (!p) return SARX_OK;
    hipSetDevice(p->ctx->device);
    sync_all_lanes(p->ctx);
    general_csa_destroy(p->gen);
    hipFree(p->c1); hipFree(p->c2); hipFree(p->c3);
    hipFree(p->ati_part);
    hipFree(p->buf_a); hipFree(p->buf_b); hipFree(p->h_in); hipFree(p->h_out); hipFree(p->look_part);
    for (int i = 0; i < sarx_plan::PIPE; ++i)             // frames still in the pipeline: their download slots go back to the ctx
        if (p->pipe_dl[i] >= 0 && p->pipe_dl[i] < sarx_ctx::DL_SLOTS) { sarx_memcpy_d2h_end(p->ctx, p->pipe_dl[i]); p->pipe_dl[i] = -1; }
    if (p->ctx->dl_stream) hipStreamSynchronize(p->ctx->dl_stream);
    for (int i = 0; i < sarx_plan::PIPE; ++i) { hipFree(p->pipe_in[i]); hipFree(p->pipe_out[i]); }
    delete p;
    return SARX_OK;
}

int sarx_csa_plan_mark_range(sarx_plan* p, int slot_start, int slot_stop) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    if (slot_start >= N_EVENTS || slot_stop >= N_EVENTS) return fail(p->ctx, SARX_ERR_INVALID, "event slot out of range");
    p->mark_start = slot_start; p->mark_stop = slot_stop;
    return SARX_OK;
}

int sarx_csa_plan_stamp_range(sarx_plan* p, uint64_t* d_pair) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    if (((uintptr_t)d_pair) & 7) return fail(p->ctx, SARX_ERR_INVALID, "the stamp pair must be 8-byte aligned");
    p->stamp = reinterpret_cast<unsigned long long*>(d_pair);
    return SARX_OK;
}

int sarx_csa_plan_set_look_slot(sarx_plan* p, int looks, float* d_slot) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!d_slot) { p->look_slot = nullptr; return SARX_OK; }            // switch off; the partials buffer is kept
    if (p->gen) return fail(c, SARX_ERR_UNSUPPORTED, "the fused stack slot exists for power-of-two plans only (use sarx_multilook_dev)");
    if (looks < 1 || (looks & (looks - 1)) || looks > p->az_w || p->n_az % looks || p->n_rg % looks)
        return fail(c, SARX_ERR_UNSUPPORTED, "looks=%d must be a power of two <= %d dividing n_az=%d and n_rg=%d", looks, p->az_w, p->n_az, p->n_rg);
    if (p->look_part && p->look != looks) { hipStreamSynchronize(c->stream); hipFree(p->look_part); p->look_part = nullptr; }
    if (!p->look_part) {
        const size_t bytes = (size_t)p->n_az * (p->n_rg / looks) * sizeof(float);
        hipError_t e = hipMalloc(&p->look_part, bytes);
        if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc look partials: %s", hipGetErrorString(e));
        p->bytes += bytes;
    }
    p->look = looks; p->look_slot = d_slot;
    return SARX_OK;
}

int sarx_csa_plan_set_max_slot(sarx_plan* p, float* d_max) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    if (p->gen && !general_csa_set_max_slot(p->gen, reinterpret_cast<unsigned*>(d_max)))
        return fail(p->ctx, SARX_ERR_UNSUPPORTED, "the fused maximum exists for power-of-two plans and 7199 x 13200 (sarx_ati_dpca_dev reduces it otherwise)");
    p->max_slot = d_max;
    return SARX_OK;
}

int sarx_csa_plan_set_ati(sarx_plan* p, const void* d_slc1, const float* d_max, float mask_frac, double cal_phase,
                          float* d_ati_phase_masked, float* d_slc1_mag, float* d_dpca_mag, int keep_image) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!d_slc1) {
        p->ati_s1 = nullptr;
        if (p->gen) general_csa_set_ati(p->gen, nullptr);
        return SARX_OK;
    }
    if (!d_max || !d_ati_phase_masked || !d_slc1_mag || !d_dpca_mag) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    if (p->gen) {        // the native 7199 x 13200: the inverse DFT-23 launch of the prime-factor route has the same epilogue
        const int parts = general_csa_ati_parts(p->gen);
        if (parts < 0 || (p->flags & SARX_OUT_RG_MAJOR))
            return fail(c, SARX_ERR_UNSUPPORTED, "the fused ATI products exist for power-of-two plans and 7199 x 13200 in the default image "
                                                 "layout (sarx_ati_dpca_dev otherwise)");
        if (!p->ati_part) {
            hipError_t e = hipMalloc(&p->ati_part, ((size_t)parts + 128) * sizeof(double2));
            if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc ATI partial sums: %s", hipGetErrorString(e));
            p->bytes += (size_t)parts * sizeof(double2);
        }
        p->ati_nparts = parts;
        AtiFuse f{};
        f.s1 = (const float2*)d_slc1; f.phase = d_ati_phase_masked; f.m1 = d_slc1_mag; f.dm = d_dpca_mag; f.part = p->ati_part;
        f.thr = d_max; f.cc = (float)cos(cal_phase); f.cs = (float)sin(cal_phase); f.frac = mask_frac; f.keep_image = keep_image != 0;
        general_csa_set_ati(p->gen, &f);
        p->ati_s1 = f.s1; p->ati_thr = d_max;
        return SARX_OK;
    }
    if (p->n_rg % 32 || (p->flags & SARX_OUT_RG_MAJOR) || p->slab_tiles > 0)
        return fail(c, SARX_ERR_UNSUPPORTED, "the fused ATI products exist for power-of-two plans in the default image layout (sarx_ati_dpca_dev otherwise)");
    int w = (p->n_rg % 64 == 0) ? 64 : 32;          // 64 columns where n_rg allows: 256-byte row segments of the fp32 planes
    if (const char* ev = getenv("SARX_ATI_W")) { const int e = atoi(ev); if ((e == 32 || e == 64) && p->n_rg % e == 0) w = e; }
    const int tpt = (p->az_s >= 16 ? p->az_s / 16 : 1) * w;        // threads per tile of the last azimuth launch (rows az_s)
    if (tpt % 64) return fail(c, SARX_ERR_UNSUPPORTED, "n_az=%d n_rg=%d: the last azimuth launch's tiles have %d threads, the fused ATI "
                                                        "products need whole waves (sarx_ati_dpca_dev otherwise)", p->n_az, p->n_rg, tpt);
    p->ati_w = w;
    const int tiles = (p->az_s == p->n_az ? 1 : p->n_az / p->az_s) * (p->n_rg / w);
    const int waves = tpt / 64;
    if (!p->ati_part) {
        hipError_t e = hipMalloc(&p->ati_part, ((size_t)tiles * waves + 128) * sizeof(double2));     // + the finish's first-level results
        if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc ATI partial sums: %s", hipGetErrorString(e));
        p->bytes += (size_t)tiles * waves * sizeof(double2);
    }
    p->ati_nparts = tiles * waves;
    p->ati_s1 = (const float2*)d_slc1; p->ati_thr = d_max; p->ati_frac = mask_frac; p->ati_cal = cal_phase;
    p->ati_phase = d_ati_phase_masked; p->ati_m1 = d_slc1_mag; p->ati_dm = d_dpca_mag; p->ati_keep_image = keep_image != 0;
    return SARX_OK;
}

int sarx_csa_plan_bytes(const sarx_plan* p, uint64_t* out) {
    if (!p || !out) return fail(p ? p->ctx : nullptr, SARX_ERR_INVALID, "NULL argument");
    *out = p->bytes;
    return SARX_OK;
}

int sarx_csa_axes(const sarx_plan* p, double* range_axis, double* cross_range_axis) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    const double dt = 1.0 / p->p.sample_rate_hz;
    if (range_axis)
        for (int j = 0; j < p->n_rg; ++j) range_axis[j] = C_LIGHT * (p->p.t_start_fast_s + (double)j * dt) / 2.0;   // :219,346
    if (cross_range_axis) {
        // t_slow = arange/prf; t_slow -= mean; * Vr   (:392-394), pairwise mean like NumPy is not
        // needed: the reference result is reproduced to 1e-13 relative, stated in the test
        double mean = 0.0;
        for (int i = 0; i < p->n_az; ++i) mean += (double)i / p->p.prf_hz;
        mean /= (double)p->n_az;
        for (int i = 0; i < p->n_az; ++i) cross_range_axis[i] = ((double)i / p->p.prf_hz - mean) * p->p.platform_speed_mps;
    }
    return SARX_OK;
}

static RangeArgs range_args(const sarx_plan* p, const void* in, void* out) {
    RangeArgs a{};
    a.in = (const float2*)in; a.out = (float2*)out;
    a.tw = p->ctx->tw_all + p->n_rg;
    a.c2 = p->c2; a.c3 = p->c3;
    a.dt = 1.0 / p->p.sample_rate_hz;
    a.df = 1.0 / ((double)p->n_rg * a.dt);           // numpy.fft.fftfreq step
    a.t_start = p->p.t_start_fast_s;
    a.t0 = 2.0 * p->p.range_ref_m / C_LIGHT;
    a.inv_n = 1.0f / (float)p->n_rg;
    a.n_az = p->n_az;
    return a;
}

// what every azimuth launch of a plan receives; the callers add the step's twiddles and strides
static AzArgs az_args(const sarx_plan* p, const void* in, void* out) {
    AzArgs a{};
    a.tw_n = p->ctx->tw_all + p->n_az;
    a.c1 = p->c1;
    a.dt = 1.0 / p->p.sample_rate_hz;
    a.t_start = p->p.t_start_fast_s;
    a.scale = 1.0f / (float)p->n_az;
    a.n_rg = p->n_rg;
    a.in = (const float2*)in; a.out = (float2*)out;
    a.nt = p->az_nt;
    return a;
}

static hipError_t run_range(const sarx_plan* p, int mode, const RangeArgs& a) {
    const sarx_ctx* c = p->ctx;
    // measured on MI355X (profiles/): 32 pts/thread wins for one FFT per launch at n_rg >= 8192,
    // 16 pts/thread wins for the fused FFT+IFFT launch (the 32-pt form spills there)
    const bool v2 = range_v2_supported(p->n_rg, mode) &&
                    (c->range_impl == 2 || (c->range_impl == 0 && p->n_rg >= 16384 && mode != RG_FUSED));
    // impl 3 (default for the fused launch at 16384): wave-private sub-transforms
    if (mode == RG_FUSED && range_fused_wl_supported(p->n_rg) && (c->range_impl == 3 || c->range_impl == 0))
        return launch_range_fused_wl(a, (c->range_cus > 0 && c->range_cus < c->cus) ? c->range_cus : c->cus, c->stream,
                                     /*alone=*/!(c->range_cus > 0 && c->range_cus < c->cus));
    return v2 ? launch_range_pass_v2(p->n_rg, mode, a, c->cus, c->stream) : launch_range_pass(p->n_rg, mode, a, c->stream);
}

static void ati_args(const sarx_plan* p, AzArgs& a) {
    a.ati_s1 = p->ati_s1; a.ati_thr = p->ati_thr; a.ati_frac = p->ati_frac;
    a.ati_cc = (float)cos(p->ati_cal); a.ati_cs = (float)sin(p->ati_cal);
    a.ati_phase = p->ati_phase; a.ati_m1 = p->ati_m1; a.ati_dm = p->ati_dm;
    a.ati_part = p->ati_part; a.ati_keep_image = p->ati_keep_image;
}
// the fixed-order finish of the fused ATI products' phase-balance sum, after the last azimuth launch of a focus
static int ati_finish(sarx_plan* p) {
    if (!p->ati_s1) return SARX_OK;
    sarx_ctx* c = p->ctx;
    HIPCHK(c, launch_ati_finish_sums(p->ati_part, p->ati_nparts, p->ati_thr, p->ati_part + p->ati_nparts, c->ati_out3_(), c->stream));
    return SARX_OK;
}
// The last launch of an azimuth transform: Phi_1 forward; inverse, the scaling with whatever the plan has armed (look slot, max slot,
// ATI products - the ATI epilogue takes precedence).  Fills those fields of `a`; returns the epilogue and the tile width that goes
// with it (w_plain: the width of a launch without look partials or ATI planes).
struct AzLast { int epi, w; };
static AzLast az_last(const sarx_plan* p, bool inv, int w_plain, AzArgs& a) {
    const bool look = inv && p->look_slot;
    if (look) { a.look_part = p->look_part; a.look = p->look; }
    const bool ati = inv && p->ati_s1;
    if (inv && !ati) a.max_out = reinterpret_cast<unsigned*>(p->max_slot);      // an armed ATI epilogue reads the slot (ati_thr): never reduce into it then
    if (ati) ati_args(p, a);
    return {inv ? (ati ? AZ_EPI_SCALE_ATI : look ? AZ_EPI_SCALE_LOOK : AZ_EPI_SCALE) : AZ_EPI_PHI1, ati ? p->ati_w : look ? p->az_w : w_plain};
}
// One step of the two-step (four-step) azimuth transform n_az = RA * S over the tiles [q0, q0 + nq):
//   step A: tile q in [0,S):  rows q + m*S, (I)FFT over m (length RA), twiddle W_n^(-+q*m'), same rows of `out`
//   step B: tile q in [0,RA): rows q*S + m, (I)FFT over m (length S), rows q + m'*RA of `out` (natural bin order), epilogue
static int az_step(sarx_plan* p, bool inv, bool step_b, int S, const void* in, void* out, int q0, int nq) {
    sarx_ctx* c = p->ctx;
    const int n = p->n_az, RA = n / S;
    AzArgs a = az_args(p, in, out);
    a.q0 = q0;
    const bool alone = !(c->range_cus > 0 && c->range_cus < c->cus);
    const int w_plain = (alone && p->az_w_alone) ? p->az_w_alone : p->az_w;      // the same columns' arithmetic either way: bit-identical images
    // wave-private 128-point tiles: chosen by the plan alone (not by the CU share), so every mode runs the same arithmetic
    const auto wave = [&](int r, int epi) { return p->az_impl && n == 16384 && az_wave_supported(r, p->n_rg, epi, p->az_wpb); };
    if (!step_b) {
        a.tw_r = c->tw_all + RA;
        a.in_q_stride = 1; a.in_m_stride = S; a.out_q_stride = 1; a.out_m_stride = S;
        if (wave(RA, AZ_EPI_TWIDDLE)) HIPCHK(c, launch_az_wave(inv, AZ_EPI_TWIDDLE, p->az_wpb, a, nq, c->stream));
        else HIPCHK(c, launch_az_tile(RA, w_plain, inv, AZ_EPI_TWIDDLE, a, nq, c->stream));
    } else {
        a.tw_r = c->tw_all + S;
        a.in_q_stride = S; a.in_m_stride = 1; a.out_q_stride = 1; a.out_m_stride = RA;
        const AzLast l = az_last(p, inv, w_plain, a);
        if (wave(S, l.epi)) HIPCHK(c, launch_az_wave(inv, l.epi, p->az_wpb, a, nq, c->stream));
        else HIPCHK(c, launch_az_tile(S, l.w, inv, l.epi, a, nq, c->stream));
    }
    return SARX_OK;
}
// the finish half of the fused multilook, after the last azimuth launch of a focus
static int look_finish(sarx_plan* p) {
    if (!p->look_slot || p->ati_s1) return SARX_OK;      // the ATI epilogue takes precedence: no look partials were written
    sarx_ctx* c = p->ctx;
    HIPCHK(c, launch_look_finish(p->look_part, p->look_slot, p->n_az / p->look, p->n_rg / p->look, p->look, c->stream));
    return SARX_OK;
}

// azimuth FFT (+epilogue) in -> out via tmp (tmp unused for single-step sizes); in is not modified
static int az_pass(sarx_plan* p, bool inv, const void* in, void* tmp, void* out) {
    sarx_ctx* c = p->ctx;
    const int n = p->n_az, S = p->az_s;
    if (S == n) {          // one tile spans the whole azimuth extent
        AzArgs a = az_args(p, in, out);
        a.tw_r = c->tw_all + n;
        a.in_q_stride = 0; a.in_m_stride = 1; a.out_q_stride = 0; a.out_m_stride = 1;
        const AzLast l = az_last(p, inv, p->az_w, a);
        HIPCHK(c, launch_az_tile(n, l.w, inv, l.epi, a, 1, c->stream));
        return SARX_OK;
    }
    int rc;
    if ((rc = az_step(p, inv, false, S, in, tmp, 0, S)) != SARX_OK) return rc;
    return az_step(p, inv, true, S, tmp, out, 0, n / S);
}

int sarx_csa_pass(sarx_plan* p, int pass_id, const void* d_in, void* d_out) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!d_in || !d_out) return fail(c, SARX_ERR_INVALID, "NULL image pointer");
    int rc;
    if (p->gen) {      // any-size plans: the range passes of a direct mixed-radix line length (13200) only
        int mode = -1;
        switch (pass_id) {
            case SARX_PASS_RG_FFT_PHI2: mode = RG_FFT_PHI2; break;
            case SARX_PASS_RG_IFFT_PHI3: mode = RG_IFFT_PHI3; break;
            case SARX_PASS_RG_FUSED_23: mode = RG_FUSED; break;
            case 100: mode = RG_FFT; break;
            case 101: mode = RG_IFFT; break;
        }
        hipError_t e = hipErrorNotSupported;
        if (mode >= 0) e = general_csa_range_pass(p->gen, mode, (const float2*)d_in, (float2*)d_out, c->stream);
        else if (pass_id == SARX_PASS_AZ_FFT_PHI1 || pass_id == SARX_PASS_AZ_IFFT) {
            if (d_in == d_out) return fail(c, SARX_ERR_INVALID, "azimuth passes are out-of-place");
            if (pass_id == SARX_PASS_AZ_IFFT && (p->max_slot || p->ati_s1))
                return fail(c, SARX_ERR_UNSUPPORTED, "the per-pass azimuth IFFT of a 7199 x 13200 plan has no max-slot / ATI epilogue: switch them off or use sarx_csa_focus_dev");
            e = general_csa_az_pass(p->gen, pass_id == SARX_PASS_AZ_IFFT, (const float2*)d_in, (float2*)d_out, c->stream);
        }
        if (e == hipErrorNotSupported)
            return fail(c, SARX_ERR_UNSUPPORTED, "per-pass entry points exist for power-of-two plans, for the range passes of n_rg = 13200 "
                                                 "and for the azimuth passes of 7199 x 13200");
        HIPCHK(c, e);
        return SARX_OK;
    }
    switch (pass_id) {
        case SARX_PASS_AZ_FFT_PHI1:
        case SARX_PASS_AZ_IFFT:
            if (d_in == d_out || d_in == p->buf_b || d_out == p->buf_b)
                return fail(c, SARX_ERR_INVALID, "azimuth passes are out-of-place");
            if (p->max_slot && !p->ati_s1 && pass_id == SARX_PASS_AZ_IFFT) HIPCHK(c, hipMemsetAsync(p->max_slot, 0, MAX_SLOT_BYTES, c->stream));
            if ((rc = az_pass(p, pass_id == SARX_PASS_AZ_IFFT, d_in, p->buf_b, d_out)) != SARX_OK) return rc;
            if (pass_id == SARX_PASS_AZ_IFFT) {      // the armed epilogues of the last azimuth launch need their finish launches here too
                if ((rc = look_finish(p)) != SARX_OK) return rc;
                if ((rc = ati_finish(p)) != SARX_OK) return rc;
            }
            return SARX_OK;
        case SARX_PASS_RG_FFT_PHI2: { RangeArgs a = range_args(p, d_in, d_out); HIPCHK(c, run_range(p, RG_FFT_PHI2, a)); return SARX_OK; }
        case SARX_PASS_RG_IFFT_PHI3: { RangeArgs a = range_args(p, d_in, d_out); HIPCHK(c, run_range(p, RG_IFFT_PHI3, a)); return SARX_OK; }
        case SARX_PASS_RG_FUSED_23: { RangeArgs a = range_args(p, d_in, d_out); HIPCHK(c, run_range(p, RG_FUSED, a)); return SARX_OK; }
        case SARX_PASS_RG_FFT_PHI2_PERM:
        case SARX_PASS_RG_IFFT_PHI3_PERM: {
            if (!range_wp_supported(p->n_rg)) return fail(c, SARX_ERR_UNSUPPORTED, "the permuted-spectrum range passes exist for n_rg = 16384 only");
            RangeArgs a = range_args(p, d_in, d_out);
            HIPCHK(c, launch_range_wp(pass_id == SARX_PASS_RG_FFT_PHI2_PERM ? RG_FFT_PHI2 : RG_IFFT_PHI3, a, c->cus, c->stream));
            return SARX_OK;
        }
        case 110: case 111: case 112: case 113: {     // one step of a four-step azimuth transform (tests): forward A, B, inverse A, B
            if (p->az_s == p->n_az || d_in == d_out || d_in == p->buf_b || d_out == p->buf_b)
                return fail(c, SARX_ERR_INVALID, "azimuth steps exist for four-step plans and are out-of-place");
            const bool inv = pass_id >= 112, step_b = pass_id & 1;
            if (inv && step_b && p->max_slot && !p->ati_s1) HIPCHK(c, hipMemsetAsync(p->max_slot, 0, MAX_SLOT_BYTES, c->stream));
            return az_step(p, inv, step_b, p->az_s, d_in, d_out, 0, step_b ? p->n_az / p->az_s : p->az_s);
        }
        case 100: { RangeArgs a = range_args(p, d_in, d_out); HIPCHK(c, run_range(p, RG_FFT, a)); return SARX_OK; }   // plain FFT (tests)
        case 101: { RangeArgs a = range_args(p, d_in, d_out); HIPCHK(c, run_range(p, RG_IFFT, a)); return SARX_OK; }  // plain IFFT (tests)
    }
    return fail(c, SARX_ERR_INVALID, "unknown pass id %d", pass_id);
}

int sarx_csa_focus_dev(sarx_plan* p, const void* d_phist, void* d_image) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!d_phist || !d_image || d_phist == d_image) return fail(c, SARX_ERR_INVALID, "image pointers NULL or aliased");
    if (p->ati_s1 && (d_image == (const void*)p->ati_s1 || d_phist == (const void*)p->ati_s1))
        return fail(c, SARX_ERR_INVALID, "the first channel's image (sarx_csa_plan_set_ati) must not be this focus's input or output: the output buffer is scratch");
    const bool rg_major = p->flags & SARX_OUT_RG_MAJOR;
    int rc;
    // the slot is cleared and re-reduced by every focus EXCEPT one with the ATI epilogue armed: that focus is the second
    // channel's and reads the first channel's maximum from it (normally the same buffer) - clearing it there made the
    // threshold 0 and the mask pass every pixel
    if (p->max_slot && !p->ati_s1) HIPCHK(c, hipMemsetAsync(p->max_slot, 0, MAX_SLOT_BYTES, c->stream));
    if (p->gen) {
        float2* dst = rg_major ? p->buf_a : (float2*)d_image;
        HIPCHK(c, general_csa_focus(p->gen, (const float2*)d_phist, dst, c->stream));
        if ((rc = ati_finish(p)) != SARX_OK) return rc;
        if (rg_major) HIPCHK(c, launch_corner_turn(p->buf_a, (float2*)d_image, p->n_az, p->n_rg, c->stream));
        return SARX_OK;
    }
    if (p->slab_tiles > 0 && p->az_s != p->n_az && (p->flags & SARX_FUSE_RANGE)) {
        // Slab mode.  The forward transform's second step, the fused range pass and the inverse transform's first step all
        // work on the same row set when the inverse is split the other way round (its stride = the forward's tile count):
        // forward tile q writes rows q + m'*RA (m' < S), the range pass needs whole rows, inverse tile q reads rows
        // q + m*RA.  Running the three launches group of tiles by group of tiles keeps a group's rows (slab_tiles * S rows)
        // in the 256 MiB Infinity Cache between them: the image makes three HBM round trips instead of five.
        const int S = p->az_s, RA = p->n_az / S, Q = p->slab_tiles;
        float2* last = rg_major ? p->buf_a : (float2*)d_image;
        if ((rc = az_step(p, false, false, S, d_phist, d_image, 0, S)) != SARX_OK) return rc;       // forward step A, whole image
        bool marked = false;
        for (int q0 = 0; q0 < RA; q0 += Q) {
            const int nq = (q0 + Q <= RA) ? Q : RA - q0;
            if ((rc = az_step(p, false, true, S, d_image, p->buf_b, q0, nq)) != SARX_OK) return rc;
            RangeArgs a = range_args(p, p->buf_b, p->buf_b);
            a.n_az = nq * S; a.row0 = q0; a.row_inner = nq; a.row_stride = RA;
            const bool mark = !marked && p->mark_start >= 0;          // the first group's launch is the one that is timed
            if (mark) { HIPCHK(c, hipEventRecord(c->ev[p->mark_start], c->stream)); c->ev_set[p->mark_start] = true; }
            HIPCHK(c, run_range(p, RG_FUSED, a));
            if (mark && p->mark_stop >= 0) { HIPCHK(c, hipEventRecord(c->ev[p->mark_stop], c->stream)); c->ev_set[p->mark_stop] = true; marked = true; }
            if ((rc = az_step(p, true, false, RA, p->buf_b, p->buf_b, q0, nq)) != SARX_OK) return rc;   // inverse step A, stride RA
        }
        if ((rc = az_step(p, true, true, RA, p->buf_b, last, 0, S)) != SARX_OK) return rc;           // inverse step B, whole image
        if ((rc = look_finish(p)) != SARX_OK) return rc;
        if (rg_major) HIPCHK(c, launch_corner_turn(p->buf_a, (float2*)d_image, p->n_az, p->n_rg, c->stream));
        return SARX_OK;
    }
    // pass 1: azimuth FFT + Phi_1: phist -> (image as step-A scratch) -> buf_b
    if ((rc = az_pass(p, false, d_phist, d_image, p->buf_b)) != SARX_OK) return rc;
    // passes 2, 3 in place on buf_b
    if (p->mark_start >= 0) { HIPCHK(c, hipEventRecord(c->ev[p->mark_start], c->stream)); c->ev_set[p->mark_start] = true; }
    if (p->flags & SARX_FUSE_RANGE) {
        RangeArgs a = range_args(p, p->buf_b, p->buf_b);
        a.stamp = p->stamp;
        HIPCHK(c, run_range(p, RG_FUSED, a));
    } else if (range_wp_supported(p->n_rg) && (c->range_impl == 0 || c->range_impl == 4)) {
        // two launches with the spectrum in permuted order between them (range_wp.hip): one workgroup-wide exchange each
        RangeArgs a = range_args(p, p->buf_b, p->buf_b);
        HIPCHK(c, launch_range_wp(RG_FFT_PHI2, a, c->cus, c->stream));
        HIPCHK(c, launch_range_wp(RG_IFFT_PHI3, a, c->cus, c->stream));
    } else {
        RangeArgs a = range_args(p, p->buf_b, p->buf_b);
        HIPCHK(c, run_range(p, RG_FFT_PHI2, a));
        HIPCHK(c, run_range(p, RG_IFFT_PHI3, a));
    }
    if (p->mark_stop >= 0) { HIPCHK(c, hipEventRecord(c->ev[p->mark_stop], c->stream)); c->ev_set[p->mark_stop] = true; }
    // pass 4: azimuth IFFT; step A in place on buf_b, step B out to the image (or buf_a before the corner turn)
    float2* last = rg_major ? p->buf_a : (float2*)d_image;
    if (p->az_s == p->n_az) {
        if ((rc = az_pass(p, true, p->buf_b, nullptr, last)) != SARX_OK) return rc;
    } else {
        if ((rc = az_pass(p, true, p->buf_b, p->buf_b, last)) != SARX_OK) return rc;
    }
    if ((rc = look_finish(p)) != SARX_OK) return rc;
    if ((rc = ati_finish(p)) != SARX_OK) return rc;
    if (rg_major) HIPCHK(c, launch_corner_turn(p->buf_a, (float2*)d_image, p->n_az, p->n_rg, c->stream));
    return SARX_OK;
}


int sarx_csa_focus_host_c128(sarx_plan* p, const void* phist_host, void* image_host) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!phist_host || !image_host) return fail(c, SARX_ERR_INVALID, "NULL host pointer");
    const size_t img = (size_t)p->n_az * p->n_rg * sizeof(float2);
    if (!p->h_in) { hipError_t e = hipMalloc(&p->h_in, img); if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc staging: %s", hipGetErrorString(e)); }
    if (!p->h_out) { hipError_t e = hipMalloc(&p->h_out, img); if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc staging: %s", hipGetErrorString(e)); }
    HIPCHK(c, staged_copy(c, p->h_in, phist_host, img, true, true));
    int rc = sarx_csa_focus_dev(p, p->h_in, p->h_out);
    if (rc != SARX_OK) return rc;
    HIPCHK(c, staged_copy(c, image_host, p->h_out, img, false));
    return SARX_OK;
}

int sarx_csa_focus_host(sarx_plan* p, const void* phist_host, void* image_host) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!phist_host || !image_host) return fail(c, SARX_ERR_INVALID, "NULL host pointer");
    const size_t img = (size_t)p->n_az * p->n_rg * sizeof(float2);
    if (!p->h_in) { hipError_t e = hipMalloc(&p->h_in, img); if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc staging: %s", hipGetErrorString(e)); }
    if (!p->h_out) { hipError_t e = hipMalloc(&p->h_out, img); if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc staging: %s", hipGetErrorString(e)); }
    HIPCHK(c, staged_copy(c, p->h_in, phist_host, img, true));
    int rc = sarx_csa_focus_dev(p, p->h_in, p->h_out);
    if (rc != SARX_OK) return rc;
    HIPCHK(c, staged_copy(c, image_host, p->h_out, img, false));
    return SARX_OK;
}

// The host-array call as a pipeline (the loop of sar_batch_sim.py:303-331, the two back-to-back calls of sar_ati_dcpa_sim_csa.py:410-411):
// _begin uploads this frame while the previous frame focuses and downloads; _end waits for a frame's image.
int sarx_csa_focus_host_begin(sarx_plan* p, const void* phist_host, void* image_host, int* out_ticket) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (!phist_host || !image_host || !out_ticket) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    *out_ticket = -1;
    const int s = p->pipe_next;
    if (p->pipe_dl[s] != -1) return fail(c, SARX_ERR_INVALID, "%d frames are in flight on this plan: call sarx_csa_focus_host_end first", sarx_plan::PIPE);
    const size_t img = (size_t)p->n_az * p->n_rg * sizeof(float2);
    for (float2** b : {&p->pipe_in[s], &p->pipe_out[s]})
        if (!*b) { hipError_t e = hipMalloc(b, img); if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc pipeline buffer: %s", hipGetErrorString(e)); }
    // slot s last held frame i - PIPE, whose _end has returned: nothing enqueued touches these two buffers, the upload need not wait
    // for the frame that is focusing or downloading right now
    HIPCHK(c, staged_copy(c, p->pipe_in[s], phist_host, img, true, false, /*ordered=*/false));
    int rc = sarx_csa_focus_dev(p, p->pipe_in[s], p->pipe_out[s]);
    if (rc != SARX_OK) return rc;
    if (is_page_locked(image_host)) {
        int slot = -1;
        if ((rc = sarx_memcpy_d2h_begin(c, image_host, p->pipe_out[s], img, &slot)) != SARX_OK) {
            hipStreamSynchronize(c->stream);        // the focus is enqueued but the slot stays free: nothing may still touch its buffers
            return rc;
        }
        p->pipe_dl[s] = slot; p->pipe_host[s] = nullptr;
    } else {                       // a pageable result cannot be the target of an asynchronous DMA: _end downloads it (staged, blocking)
        p->pipe_dl[s] = sarx_ctx::DL_SLOTS; p->pipe_host[s] = image_host;
    }
    p->pipe_next = (s + 1) % sarx_plan::PIPE;
    *out_ticket = s;
    return SARX_OK;
}
int sarx_csa_focus_host_end(sarx_plan* p, int ticket) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    sarx_ctx* c = p->ctx;
    hipSetDevice(c->device);
    if (ticket < 0 || ticket >= sarx_plan::PIPE || p->pipe_dl[ticket] == -1) return fail(c, SARX_ERR_INVALID, "ticket %d is not in flight", ticket);
    const int slot = p->pipe_dl[ticket];
    p->pipe_dl[ticket] = -1;
    if (slot == sarx_ctx::DL_SLOTS) {
        const size_t img = (size_t)p->n_az * p->n_rg * sizeof(float2);
        HIPCHK(c, staged_copy(c, p->pipe_host[ticket], p->pipe_out[ticket], img, false));      // ordered: waits for the focus
        return SARX_OK;
    }
    return sarx_memcpy_d2h_end(c, slot);
}

}  // extern "C"
