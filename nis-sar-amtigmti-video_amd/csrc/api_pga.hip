// libsarx C ABI of include/sarx_pga.h: parameter and layout checks and the launches of pga.hip.
#include "../../include/sarx_pga.h"
#include "api_gmti.h"
#include "pga.h"

#include <cmath>

using namespace sarx;

static constexpr size_t PGA_MAX_LD = (size_t)1 << 31;          // elements per image row and between two frames' starts: the
static constexpr size_t PGA_MAX_STRIDE = (size_t)1 << 40;      // byte spans below stay far from overflow

static int pga_layout_check(sarx_ctx* c, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride) {
    if (n_az != 64 && n_az != 128 && n_az != 256 && n_az != 512 && n_az != 1024)
        return fail(c, SARX_ERR_INVALID, "PGA n_az %d: must be 64, 128, 256, 512 or 1024", n_az);
    if (n_rg < 1 || n_rg > SARX_PGA_MAX_RG) return fail(c, SARX_ERR_INVALID, "PGA n_rg %d must be 1 .. %d", n_rg, SARX_PGA_MAX_RG);
    if (ld < (size_t)n_rg || ld > PGA_MAX_LD) return fail(c, SARX_ERR_INVALID, "PGA ld %zu must be n_rg = %d .. %zu", ld, n_rg, PGA_MAX_LD);
    if (n_frames < 1 || n_frames > SARX_PGA_MAX_FRAMES)
        return fail(c, SARX_ERR_INVALID, "PGA n_frames %d must be 1 .. %d", n_frames, SARX_PGA_MAX_FRAMES);
    if (n_frames > 1 && (frame_stride < (size_t)(n_az - 1) * ld + (size_t)n_rg || frame_stride > PGA_MAX_STRIDE))
        return fail(c, SARX_ERR_INVALID, "PGA frame_stride %zu: frames of %d rows, %zu elements apart, overlap (or the stride exceeds %zu)",
                    frame_stride, n_az, ld, PGA_MAX_STRIDE);
    return SARX_OK;
}

static int pga_check(sarx_ctx* c, const sarx_pga_params* p, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride) {
    if (!p) return fail(c, SARX_ERR_INVALID, "PGA params is NULL");
    if (const int rc = pga_layout_check(c, n_az, n_rg, ld, n_frames, frame_stride)) return rc;
    if (p->n_iter < 1 || p->n_iter > SARX_PGA_MAX_ITER) return fail(c, SARX_ERR_INVALID, "PGA n_iter %d must be 1 .. %d", p->n_iter, SARX_PGA_MAX_ITER);
    for (int it = 0; it < p->n_iter; ++it)
        if (p->half_width[it] < 1 || p->half_width[it] > (n_az - 1) / 2)
            return fail(c, SARX_ERR_INVALID, "PGA half_width[%d] = %d: must be >= 1 with 2 h + 1 <= %d", it, p->half_width[it], n_az);
    if (p->reserved != 0) return fail(c, SARX_ERR_INVALID, "PGA params: reserved must be 0");
    if (!(std::isfinite(p->min_contrast) && p->min_contrast >= 0.0)) return fail(c, SARX_ERR_INVALID, "PGA min_contrast must be finite and >= 0");
    if (!(p->power_floor >= 0.0 && p->power_floor < 1.0)) return fail(c, SARX_ERR_INVALID, "PGA power_floor must be in [0, 1)");
    return SARX_OK;
}

// bytes from the first element of frame 0 to the last of frame n_frames - 1
static size_t stack_span(int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride) {
    return ((size_t)(n_frames - 1) * (n_frames > 1 ? frame_stride : 0) + (size_t)(n_az - 1) * ld + (size_t)n_rg) * sizeof(float2);
}
static size_t workspace_bytes(int n_az, int n_rg, int n_frames) {
    return (size_t)n_frames * pga_tiles(n_az, n_rg) * pga_row_doubles(n_az) * sizeof(double);
}
static PgaLayout layout(int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride) {
    return {n_az, n_rg, n_frames, ld, n_frames > 1 ? frame_stride : 0};
}

extern "C" {

int sarx_pga_check(const sarx_pga_params* p, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride) {
    return pga_check(nullptr, p, n_az, n_rg, ld, n_frames, frame_stride);
}

int sarx_pga_workspace_bytes(const sarx_pga_params* p, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride, size_t* out) {
    return size_query(out, [&] { return pga_check(nullptr, p, n_az, n_rg, ld, n_frames, frame_stride); },
                      [&] { return workspace_bytes(n_az, n_rg, n_frames); });
}

int sarx_pga_dev(sarx_ctx* c, const void* d_in, void* d_out, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride,
                 const sarx_pga_params* p, double* d_phase, sarx_pga_record* d_records, void* d_workspace) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = pga_check(c, p, n_az, n_rg, ld, n_frames, frame_stride)) return rc;
        const DevBuf bufs[] = {need(d_in, 8), need(d_out, 8), need(d_phase, 8), need(d_records, 8), need(d_workspace, 8)};
        if (const int rc = buffers_ok(c, bufs, "PGA: misaligned image, phase, records or workspace (8-byte alignment)")) return rc;
        const size_t span = stack_span(n_az, n_rg, ld, n_frames, frame_stride);
        const Span in[] = {{d_in, span}};
        const Span out[] = {{d_out, span},
                            {d_phase, (size_t)n_frames * n_az * sizeof(double)},
                            {d_records, (size_t)n_frames * (p->n_iter + 1) * sizeof(sarx_pga_record)},
                            {d_workspace, workspace_bytes(n_az, n_rg, n_frames)}};
        if (const int rc = check_spans(c, in, out, "PGA: an output overlaps the input", "PGA: two outputs overlap")) return rc;
        PgaEstimateArgs e{};
        e.g = layout(n_az, n_rg, ld, n_frames, frame_stride);
        e.min_contrast = p->min_contrast;
        e.power_floor = p->power_floor;
        e.work = (double*)d_workspace;
        e.phase = d_phase;
        e.rec_stride = p->n_iter + 1;
        PgaApplyArgs ap{};
        ap.g = e.g;
        ap.src = (const float2*)d_in;
        ap.dst = (float2*)d_out;
        ap.phase = d_phase;
        ap.phase_stride = (size_t)n_az;
        ap.sign_rev = -1.0 / (2.0 * M_PI);
        for (int it = 0; it <= p->n_iter; ++it) {
            e.src = it == 0 ? (const float2*)d_in : (const float2*)d_out;      // g_it
            e.half_width = p->half_width[it < p->n_iter ? it : p->n_iter - 1];
            e.rec = d_records + it;
            e.first = it == 0;
            e.update = it < p->n_iter;
            HIPCHK(c, launch_pga_estimate(e, c->stream));
            if (it < p->n_iter) HIPCHK(c, launch_pga_apply(ap, c->stream));
        }
        return (int)SARX_OK;
    });
}

int sarx_pga_apply_dev(sarx_ctx* c, const void* d_in, void* d_out, int n_az, int n_rg, size_t ld, int n_frames, size_t frame_stride,
                       const double* d_phase, size_t phase_stride, int sign) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = pga_layout_check(c, n_az, n_rg, ld, n_frames, frame_stride)) return rc;
        if (sign != 1 && sign != -1) return fail(c, SARX_ERR_INVALID, "PGA apply: sign %d must be -1 (correct) or +1 (inject)", sign);
        if (phase_stride != 0 && (phase_stride < (size_t)n_az || phase_stride > PGA_MAX_STRIDE))
            return fail(c, SARX_ERR_INVALID, "PGA apply: phase_stride %zu must be 0 or >= n_az = %d", phase_stride, n_az);
        const DevBuf bufs[] = {need(d_in, 8), need(d_out, 8), need(d_phase, 8)};
        if (const int rc = buffers_ok(c, bufs, "PGA apply: misaligned image or phase (8-byte alignment)")) return rc;
        const size_t span = stack_span(n_az, n_rg, ld, n_frames, frame_stride);
        const Span in[] = {{d_in, span}, {d_phase, ((size_t)(n_frames - 1) * phase_stride + (size_t)n_az) * sizeof(double)}};
        const Span out[] = {{d_out, span}};
        if (const int rc = check_spans(c, in, out, "PGA apply: the output overlaps an input", nullptr)) return rc;
        PgaApplyArgs ap{};
        ap.g = layout(n_az, n_rg, ld, n_frames, frame_stride);
        ap.src = (const float2*)d_in;
        ap.dst = (float2*)d_out;
        ap.phase = d_phase;
        ap.phase_stride = phase_stride;
        ap.sign_rev = (double)sign / (2.0 * M_PI);
        HIPCHK(c, launch_pga_apply(ap, c->stream));
        return (int)SARX_OK;
    });
}

}  // extern "C"
