// libsarx C ABI of include/sarx_balance.h: parameter checks and the launches of balance.hip.
#include "../../include/sarx_balance.h"
#include "api_gmti.h"
#include "balance.h"

#include <cfloat>
#include <cmath>

using namespace sarx;

extern "C" {

static constexpr int BALANCE_MAX_DIM = 1 << 20;      // rows / columns of an image (the apply grid has one row of workgroups per 16 image rows)

static int balance_check(sarx_ctx* c, const sarx_balance_params* p, int n_az, int n_rg) {
    if (!p) return fail(c, SARX_ERR_INVALID, "balance params is NULL");
    if (const int rc = plane_size_check(c, "image", n_az, n_rg, BALANCE_MAX_DIM, "balance")) return rc;
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
    return size_query(out, [&] { return balance_check(nullptr, p, n_az, n_rg); }, [&] {
        const BalanceGeom g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
        return table_bytes<sarx_balance_header, sarx_balance_record>((size_t)g.nb_az * g.nb_rg);
    });
}

int sarx_balance_workspace_bytes(const sarx_balance_params* p, int n_az, int n_rg, size_t* out) {
    return size_query(out, [&] { return balance_check(nullptr, p, n_az, n_rg); }, [&] {
        const BalanceGeom g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
        return (size_t)g.nb_az * g.nb_rg * g.strips * sizeof(BalPartial);
    });
}

int sarx_balance_estimate_dev(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, const sarx_balance_params* p,
                              void* d_table, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = balance_check(c, p, n_az, n_rg)) return rc;
        if (const int rc = buffers_ok(c, {need(d_slc1, 8), need(d_slc2, 8), need(d_table, 8), need(d_workspace, 8)},
                                      "misaligned image, table or workspace (8-byte alignment)"))
            return rc;
        BalanceEstimateArgs a{};
        a.s1 = (const float2*)d_slc1; a.s2 = (const float2*)d_slc2;
        a.g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
        a.clip = std::fmin((float)p->clip_power, FLT_MAX);
        a.mode = p->mode; a.min_count = p->min_count; a.min_coherence = p->min_coherence;
        a.part = (BalPartial*)d_workspace;
        a.hdr = (sarx_balance_header*)d_table;
        a.rec = records_of<sarx_balance_header, sarx_balance_record>(d_table);
        HIPCHK(c, launch_balance_estimate(a, c->stream));
        return (int)SARX_OK;
    });
}

int sarx_balance_apply_dev(sarx_ctx* c, const void* d_slc1, const void* d_slc2, int n_az, int n_rg, const sarx_balance_params* p,
                           const void* d_table, void* d_slc2_out, float* d_dpca_mag) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = balance_check(c, p, n_az, n_rg)) return rc;
        const DevBuf bufs[] = {opt(d_slc1, 8), need(d_slc2, 8), need(d_table, 8), need(d_slc2_out, 8), opt(d_dpca_mag, 4)};
        if (const int rc = buffers_present(c, bufs)) return rc;
        if (d_dpca_mag && !d_slc1) return fail(c, SARX_ERR_INVALID, "dpca_mag needs slc1");
        if (const int rc = buffers_aligned(c, bufs, "misaligned image, table (8-byte alignment) or dpca_mag (4-byte alignment)")) return rc;
        BalanceApplyArgs a{};
        a.s1 = d_dpca_mag ? (const float2*)d_slc1 : nullptr;
        a.s2 = (const float2*)d_slc2;
        a.out = (float2*)d_slc2_out;
        a.dm = d_dpca_mag;
        a.g = balance_geom(n_az, n_rg, p->block_az, p->block_rg);
        a.interp = p->interp;
        a.rec = records_of<sarx_balance_header, const sarx_balance_record>(d_table);
        HIPCHK(c, launch_balance_apply(a, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
