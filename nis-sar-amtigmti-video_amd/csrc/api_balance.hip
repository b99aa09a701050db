// libsarx C ABI of include/sarx_balance.h: parameter checks and the launches of balance.hip.
#include "../../include/sarx_balance.h"
#include "api_ctx.h"
#include "balance.h"

#include <cfloat>
#include <cmath>

using namespace sarx;

extern "C" {

static constexpr int BALANCE_MAX_DIM = 1 << 20;      // rows / columns of an image (the apply grid has one row of workgroups per 16 image rows)

static int balance_check(sarx_ctx* c, const sarx_balance_params* p, int n_az, int n_rg) {
    if (!p) return fail(c, SARX_ERR_INVALID, "balance params is NULL");
    if (n_az < 1 || n_rg < 1) return fail(c, SARX_ERR_INVALID, "bad image size %d x %d", n_az, n_rg);
    if (n_az > BALANCE_MAX_DIM || n_rg > BALANCE_MAX_DIM)
        return fail(c, SARX_ERR_UNSUPPORTED, "balance image size %d x %d exceeds %d per side", n_az, n_rg, BALANCE_MAX_DIM);
    if (p->block_az < SARX_BALANCE_MIN_BLOCK || p->block_az > SARX_BALANCE_MAX_BLOCK || p->block_rg < SARX_BALANCE_MIN_BLOCK ||
        p->block_rg > SARX_BALANCE_MAX_BLOCK)
        return fail(c, SARX_ERR_INVALID, "balance block %d x %d: each side must be %d .. %d", p->block_az, p->block_rg,
                    SARX_BALANCE_MIN_BLOCK, SARX_BALANCE_MAX_BLOCK);
    const BalanceGeom g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
    if ((long long)g.nb_az * g.nb_rg > SARX_BALANCE_MAX_BLOCKS)
        return fail(c, SARX_ERR_UNSUPPORTED, "balance: %d x %d blocks exceed %d", g.nb_az, g.nb_rg, SARX_BALANCE_MAX_BLOCKS);
    if (p->mode != SARX_BALANCE_LS && p->mode != SARX_BALANCE_PHASE) return fail(c, SARX_ERR_INVALID, "balance mode %d unknown", p->mode);
    if (p->interp != SARX_BALANCE_NEAREST && p->interp != SARX_BALANCE_BILINEAR)
        return fail(c, SARX_ERR_INVALID, "balance interp %d unknown", p->interp);
    if (p->min_count < 1) return fail(c, SARX_ERR_INVALID, "balance min_count must be >= 1");
    if (p->reserved != 0) return fail(c, SARX_ERR_INVALID, "balance params: reserved must be 0");
    if (!(p->clip_power > 0.0)) return fail(c, SARX_ERR_INVALID, "balance clip_power must be > 0 (+inf = no clip)");
    if (!(p->min_coherence >= 0.0 && p->min_coherence <= 1.0)) return fail(c, SARX_ERR_INVALID, "balance min_coherence must lie in 0 .. 1");
    return SARX_OK;
}

int sarx_balance_check(const sarx_balance_params* p, int n_az, int n_rg) { return balance_check(nullptr, p, n_az, n_rg); }

int sarx_balance_table_bytes(const sarx_balance_params* p, int n_az, int n_rg, size_t* out) {
    if (!out) return fail(nullptr, SARX_ERR_INVALID, "out_bytes is NULL");
    const int rc = balance_check(nullptr, p, n_az, n_rg);
    if (rc != SARX_OK) return rc;
    const BalanceGeom g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
    *out = sizeof(sarx_balance_header) + (size_t)g.nb_az * g.nb_rg * sizeof(sarx_balance_record);
    return SARX_OK;
}

int sarx_balance_workspace_bytes(const sarx_balance_params* p, int n_az, int n_rg, size_t* out) {
    if (!out) return fail(nullptr, SARX_ERR_INVALID, "out_bytes is NULL");
    const int rc = balance_check(nullptr, p, n_az, n_rg);
    if (rc != SARX_OK) return rc;
    const BalanceGeom g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
    *out = (size_t)g.nb_az * g.nb_rg * g.strips * sizeof(BalPartial);
    return SARX_OK;
}

int sarx_balance_estimate_dev(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, const sarx_balance_params* p,
                              void* d_table, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        const int rc = balance_check(c, p, n_az, n_rg);
        if (rc != SARX_OK) return rc;
        if (!d_slc1 || !d_slc2 || !d_table || !d_workspace) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
        if (((uintptr_t)d_slc1 & 7) || ((uintptr_t)d_slc2 & 7) || ((uintptr_t)d_table & 7) || ((uintptr_t)d_workspace & 7))
            return fail(c, SARX_ERR_INVALID, "misaligned image, table or workspace (8-byte alignment)");
        BalanceEstimateArgs a{};
        a.s1 = (const float2*)d_slc1; a.s2 = (const float2*)d_slc2;
        a.g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
        a.clip = std::fmin((float)p->clip_power, FLT_MAX);
        a.mode = p->mode; a.min_count = p->min_count; a.min_coherence = p->min_coherence;
        a.part = (BalPartial*)d_workspace;
        a.hdr = (sarx_balance_header*)d_table;
        a.rec = (sarx_balance_record*)((char*)d_table + sizeof(sarx_balance_header));
        HIPCHK(c, launch_balance_estimate(a, c->stream));
        return (int)SARX_OK;
    });
}

int sarx_balance_apply_dev(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, const sarx_balance_params* p,
                           const void* d_table, void* d_slc2_out, float* d_dpca_mag) {
    NEED_CTX(c);
    return guarded(c, [&] {
        const int rc = balance_check(c, p, n_az, n_rg);
        if (rc != SARX_OK) return rc;
        if (!d_slc2 || !d_table || !d_slc2_out) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
        if (d_dpca_mag && !d_slc1) return fail(c, SARX_ERR_INVALID, "dpca_mag needs slc1");
        if (((uintptr_t)d_slc1 & 7) || ((uintptr_t)d_slc2 & 7) || ((uintptr_t)d_table & 7) || ((uintptr_t)d_slc2_out & 7) ||
            ((uintptr_t)d_dpca_mag & 3))
            return fail(c, SARX_ERR_INVALID, "misaligned image, table (8-byte alignment) or dpca_mag (4-byte alignment)");
        BalanceApplyArgs a{};
        a.s1 = d_dpca_mag ? (const float2*)d_slc1 : nullptr;
        a.s2 = (const float2*)d_slc2;
        a.out = (float2*)d_slc2_out;
        a.dm = d_dpca_mag;
        a.g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
        a.interp = p->interp;
        a.rec = (const sarx_balance_record*)((const char*)d_table + sizeof(sarx_balance_header));
        HIPCHK(c, launch_balance_apply(a, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
