// libsarx C ABI of include/sarx_coherence.h: parameter checks and the launches of coherence.hip.
#include "../../include/sarx_coherence.h"
#include "api_gmti.h"
#include "coherence.h"

#include <cmath>

using namespace sarx;

extern "C" {

static constexpr int COH_MAX_DIM = 1 << 20;          // rows / columns of an image (the grid has one row of workgroups per COH_TH image rows)

static int coherence_check(sarx_ctx* c, const sarx_coherence_params* p, int n_az, int n_rg) {
    if (!p) return fail(c, SARX_ERR_INVALID, "coherence params is NULL");
    if (const int rc = plane_size_check(c, "image", n_az, n_rg, COH_MAX_DIM, "coherence")) return rc;
    if (p->ha < 0 || p->ha > SARX_COH_MAX_HALF || p->hr < 0 || p->hr > SARX_COH_MAX_HALF)
        return fail(c, SARX_ERR_INVALID, "coherence window half-widths %d, %d: each must be 0 .. %d", p->ha, p->hr, SARX_COH_MAX_HALF);
    if (p->flags != 0) return fail(c, SARX_ERR_INVALID, "coherence flags %d: none is defined", p->flags);
    if (p->reserved != 0) return fail(c, SARX_ERR_INVALID, "coherence params: reserved must be 0");
    if (!(std::isfinite(p->threshold) && p->threshold >= 0.0)) return fail(c, SARX_ERR_INVALID, "coherence threshold must be finite and >= 0");
    if (!(std::isfinite(p->power_floor) && p->power_floor >= 0.0))
        return fail(c, SARX_ERR_INVALID, "coherence power_floor must be finite and >= 0");
    return SARX_OK;
}

int sarx_coherence_check(const sarx_coherence_params* p, int n_az, int n_rg) { return coherence_check(nullptr, p, n_az, n_rg); }

static size_t workspace_bytes(int n_az, int n_rg) { return (size_t)coherence_tiles_az(n_az) * coherence_tiles_rg(n_rg) * sizeof(CohPartial); }

int sarx_coherence_workspace_bytes(const sarx_coherence_params* p, int n_az, int n_rg, size_t* out) {
    return size_query(out, [&] { return coherence_check(nullptr, p, n_az, n_rg); }, [&] { return workspace_bytes(n_az, n_rg); });
}

static const char* const VS_IN = "coherence: an output overlaps an input";
static const char* const VS_OUT = "coherence: two outputs overlap";

static int check_pointers(sarx_ctx* c, const void* d_a, const void* d_b, const float* d_coh, const void* d_igram, const void* d_summary,
                          const void* d_workspace) {
    const DevBuf bufs[] = {need(d_a, 8), need(d_b, 8), opt(d_igram, 8), opt(d_summary, 8), opt(d_workspace, 8), need(d_coh, 4)};
    if (const int rc = buffers_present(c, bufs)) return rc;
    if (d_summary && !d_workspace) return fail(c, SARX_ERR_INVALID, "coherence: a summary needs the workspace");
    return buffers_aligned(c, bufs, "misaligned image, igram, summary or workspace (8-byte alignment) or coh (4-byte alignment)");
}

static CoherenceArgs make_args(const void* d_a, const void* d_b, int n_az, int n_rg, const sarx_coherence_params* p, float* d_coh,
                               void* d_igram, uint8_t* d_mask, void* d_summary, void* d_workspace) {
    CoherenceArgs a{};
    a.a = (const float2*)d_a; a.b = (const float2*)d_b;
    a.n_az = n_az; a.n_rg = n_rg; a.ha = p->ha; a.hr = p->hr;
    a.threshold = (float)p->threshold;
    a.power_floor = p->power_floor;
    a.coh = d_coh; a.igram = (float2*)d_igram; a.mask = d_mask;
    a.summary = (sarx_coherence_summary*)d_summary;
    a.part = d_summary ? (CohPartial*)d_workspace : nullptr;
    return a;
}

int sarx_coherence_pair_dev(sarx_ctx* c, const void* d_a, const void* d_b, int n_az, int n_rg, const sarx_coherence_params* p, float* d_coh,
                            void* d_igram, uint8_t* d_mask, void* d_summary, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = coherence_check(c, p, n_az, n_rg)) return rc;
        if (const int rc = check_pointers(c, d_a, d_b, d_coh, d_igram, d_summary, d_workspace)) return rc;
        const size_t n = (size_t)n_az * n_rg;
        const size_t ws = d_summary ? workspace_bytes(n_az, n_rg) : 0;
        const Span in[] = {{d_a, n * 8}, {d_b, n * 8}};
        const Span out[] = {{d_coh, n * 4}, {d_igram, n * 8}, {d_mask, n}, {d_summary, sizeof(sarx_coherence_summary)}, {d_workspace, ws}};
        if (const int rc = check_spans(c, in, out, VS_IN, VS_OUT)) return rc;
        HIPCHK(c, launch_coherence(make_args(d_a, d_b, n_az, n_rg, p, d_coh, d_igram, d_mask, d_summary, d_workspace), c->stream));
        return (int)SARX_OK;
    });
}

int sarx_coherence_stack_dev(sarx_ctx* c, const void* d_frames, int n_frames, size_t frame_stride_bytes, int lag, int n_az, int n_rg,
                             const sarx_coherence_params* p, float* d_coh, size_t coh_stride_bytes, void* d_igram, size_t igram_stride_bytes,
                             uint8_t* d_mask, size_t mask_stride_bytes, void* d_summary, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = coherence_check(c, p, n_az, n_rg)) return rc;
        if (n_frames < 2 || lag < 1 || lag >= n_frames)
            return fail(c, SARX_ERR_INVALID, "coherence stack: %d frames with lag %d (needs 1 <= lag < n_frames)", n_frames, lag);
        if (const int rc = check_pointers(c, d_frames, d_frames, d_coh, d_igram, d_summary, d_workspace)) return rc;
        const size_t n = (size_t)n_az * n_rg;
        if (!stride_ok(frame_stride_bytes, n * 8)) return fail(c, SARX_ERR_INVALID, "coherence stack: bad frame stride");
        if (coh_stride_bytes < n * 4 || (coh_stride_bytes & 3)) return fail(c, SARX_ERR_INVALID, "coherence stack: bad coh stride");
        if (d_igram && !stride_ok(igram_stride_bytes, n * 8)) return fail(c, SARX_ERR_INVALID, "coherence stack: bad igram stride");
        if (d_mask && mask_stride_bytes < n) return fail(c, SARX_ERR_INVALID, "coherence stack: bad mask stride");
        const size_t pairs = (size_t)(n_frames - lag);
        const size_t ws = d_summary ? workspace_bytes(n_az, n_rg) : 0;
        const Span in[] = {{d_frames, (size_t)(n_frames - 1) * frame_stride_bytes + n * 8}};
        const Span out[] = {{d_coh, (pairs - 1) * coh_stride_bytes + n * 4},
                             {d_igram, d_igram ? (pairs - 1) * igram_stride_bytes + n * 8 : 0},
                             {d_mask, d_mask ? (pairs - 1) * mask_stride_bytes + n : 0},
                             {d_summary, pairs * sizeof(sarx_coherence_summary)},
                             {d_workspace, ws}};
        if (const int rc = check_spans(c, in, out, VS_IN, VS_OUT)) return rc;
        for (size_t f = 0; f < pairs; ++f) {
            const char* fa = (const char*)d_frames + f * frame_stride_bytes;
            const char* fb = (const char*)d_frames + (f + (size_t)lag) * frame_stride_bytes;
            // the workspace is shared: pair f's finish launch has read it before pair f + 1's workgroups write it (one stream)
            HIPCHK(c, launch_coherence(make_args(fa, fb, n_az, n_rg, p, (float*)((char*)d_coh + f * coh_stride_bytes),
                                                 d_igram ? (char*)d_igram + f * igram_stride_bytes : nullptr,
                                                 d_mask ? d_mask + f * mask_stride_bytes : nullptr,
                                                 d_summary ? (char*)d_summary + f * sizeof(sarx_coherence_summary) : nullptr, d_workspace),
                                       c->stream));
        }
        return (int)SARX_OK;
    });
}

}  // extern "C"
