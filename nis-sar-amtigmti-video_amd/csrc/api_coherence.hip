// libsarx C ABI of include/sarx_coherence.h: parameter checks and the launches of coherence.hip.
#include "../../include/sarx_coherence.h"
#include "api_ctx.h"
#include "coherence.h"

#include <cmath>

using namespace sarx;

extern "C" {

static constexpr int COH_MAX_DIM = 1 << 20;          // rows / columns of an image (the grid has one row of workgroups per COH_TH image rows)

static int coherence_check(sarx_ctx* c, const sarx_coherence_params* p, int n_az, int n_rg) {
    if (!p) return fail(c, SARX_ERR_INVALID, "coherence params is NULL");
    if (n_az < 1 || n_rg < 1) return fail(c, SARX_ERR_INVALID, "bad image size %d x %d", n_az, n_rg);
    if (n_az > COH_MAX_DIM || n_rg > COH_MAX_DIM)
        return fail(c, SARX_ERR_UNSUPPORTED, "coherence image size %d x %d exceeds %d per side", n_az, n_rg, COH_MAX_DIM);
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

int sarx_coherence_workspace_bytes(const sarx_coherence_params* p, int n_az, int n_rg, size_t* out) {
    if (!out) return fail(nullptr, SARX_ERR_INVALID, "out_bytes is NULL");
    const int rc = coherence_check(nullptr, p, n_az, n_rg);
    if (rc != SARX_OK) return rc;
    *out = (size_t)coherence_tiles_az(n_az) * coherence_tiles_rg(n_rg) * sizeof(CohPartial);
    return SARX_OK;
}

struct Span {
    const void* p;
    size_t n;
};

// no output may share a byte with an input or with another output
static int check_spans(sarx_ctx* c, const Span* in, int n_in, const Span* out, int n_out) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (ranges_overlap(out[o].p, out[o].n, in[i].p, in[i].n)) return fail(c, SARX_ERR_INVALID, "coherence: an output overlaps an input");
        for (int k = o + 1; k < n_out; ++k)
            if (ranges_overlap(out[o].p, out[o].n, out[k].p, out[k].n)) return fail(c, SARX_ERR_INVALID, "coherence: two outputs overlap");
    }
    return SARX_OK;
}

static int check_pointers(sarx_ctx* c, const void* d_a, const void* d_b, const float* d_coh, const void* d_igram, const void* d_summary,
                          const void* d_workspace) {
    if (!d_a || !d_b || !d_coh) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
    if (d_summary && !d_workspace) return fail(c, SARX_ERR_INVALID, "coherence: a summary needs the workspace");
    if (((uintptr_t)d_a & 7) || ((uintptr_t)d_b & 7) || ((uintptr_t)d_igram & 7) || ((uintptr_t)d_summary & 7) || ((uintptr_t)d_workspace & 7) ||
        ((uintptr_t)d_coh & 3))
        return fail(c, SARX_ERR_INVALID, "misaligned image, igram, summary or workspace (8-byte alignment) or coh (4-byte alignment)");
    return SARX_OK;
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
        int rc = coherence_check(c, p, n_az, n_rg);
        if (rc != SARX_OK) return rc;
        rc = check_pointers(c, d_a, d_b, d_coh, d_igram, d_summary, d_workspace);
        if (rc != SARX_OK) return rc;
        const size_t n = (size_t)n_az * n_rg;
        const size_t ws = d_summary ? (size_t)coherence_tiles_az(n_az) * coherence_tiles_rg(n_rg) * sizeof(CohPartial) : 0;
        const Span in[2] = {{d_a, n * 8}, {d_b, n * 8}};
        const Span out[5] = {{d_coh, n * 4}, {d_igram, n * 8}, {d_mask, n}, {d_summary, sizeof(sarx_coherence_summary)}, {d_workspace, ws}};
        rc = check_spans(c, in, 2, out, 5);
        if (rc != SARX_OK) return rc;
        HIPCHK(c, launch_coherence(make_args(d_a, d_b, n_az, n_rg, p, d_coh, d_igram, d_mask, d_summary, d_workspace), c->stream));
        return (int)SARX_OK;
    });
}

int sarx_coherence_stack_dev(sarx_ctx* c, const void* d_frames, int n_frames, size_t frame_stride_bytes, int lag, int n_az, int n_rg,
                             const sarx_coherence_params* p, float* d_coh, size_t coh_stride_bytes, void* d_igram, size_t igram_stride_bytes,
                             uint8_t* d_mask, size_t mask_stride_bytes, void* d_summary, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        int rc = coherence_check(c, p, n_az, n_rg);
        if (rc != SARX_OK) return rc;
        if (n_frames < 2 || lag < 1 || lag >= n_frames)
            return fail(c, SARX_ERR_INVALID, "coherence stack: %d frames with lag %d (needs 1 <= lag < n_frames)", n_frames, lag);
        rc = check_pointers(c, d_frames, d_frames, d_coh, d_igram, d_summary, d_workspace);
        if (rc != SARX_OK) return rc;
        const size_t n = (size_t)n_az * n_rg;
        if (frame_stride_bytes < n * 8 || (frame_stride_bytes & 7)) return fail(c, SARX_ERR_INVALID, "coherence stack: bad frame stride");
        if (coh_stride_bytes < n * 4 || (coh_stride_bytes & 3)) return fail(c, SARX_ERR_INVALID, "coherence stack: bad coh stride");
        if (d_igram && (igram_stride_bytes < n * 8 || (igram_stride_bytes & 7))) return fail(c, SARX_ERR_INVALID, "coherence stack: bad igram stride");
        if (d_mask && mask_stride_bytes < n) return fail(c, SARX_ERR_INVALID, "coherence stack: bad mask stride");
        const size_t pairs = (size_t)(n_frames - lag);
        const size_t ws = d_summary ? (size_t)coherence_tiles_az(n_az) * coherence_tiles_rg(n_rg) * sizeof(CohPartial) : 0;
        const Span in[1] = {{d_frames, (size_t)(n_frames - 1) * frame_stride_bytes + n * 8}};
        const Span out[5] = {{d_coh, (pairs - 1) * coh_stride_bytes + n * 4},
                             {d_igram, d_igram ? (pairs - 1) * igram_stride_bytes + n * 8 : 0},
                             {d_mask, d_mask ? (pairs - 1) * mask_stride_bytes + n : 0},
                             {d_summary, pairs * sizeof(sarx_coherence_summary)},
                             {d_workspace, ws}};
        rc = check_spans(c, in, 1, out, 5);
        if (rc != SARX_OK) return rc;
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
