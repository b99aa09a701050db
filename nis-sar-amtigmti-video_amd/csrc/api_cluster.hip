// libsarx C ABI of include/sarx_cluster.h: parameter checks and the launch of cluster.hip.
#include "../../include/sarx_cluster.h"
#include "api_gmti.h"
#include "cluster.h"

using namespace sarx;

extern "C" {

static int cluster_check(sarx_ctx* c, const sarx_cluster_params* p) {
    if (!p) return fail(c, SARX_ERR_INVALID, "cluster params is NULL");
    if (p->link_az < 0 || p->link_az > SARX_CLUSTER_MAX_LINK || p->link_rg < 0 || p->link_rg > SARX_CLUSTER_MAX_LINK)
        return fail(c, SARX_ERR_INVALID, "cluster link (%d, %d) must lie in 0 .. %d", p->link_az, p->link_rg, SARX_CLUSTER_MAX_LINK);
    if (p->min_members < 1) return fail(c, SARX_ERR_INVALID, "cluster min_members %d must be >= 1", p->min_members);
    if (p->max_detections < 1 || p->max_detections > SARX_CLUSTER_MAX_DETECTIONS)
        return fail(c, SARX_ERR_INVALID, "cluster max_detections %d must be 1 .. %d", p->max_detections, SARX_CLUSTER_MAX_DETECTIONS);
    return SARX_OK;
}

int sarx_cluster_check(const sarx_cluster_params* p) { return cluster_check(nullptr, p); }

static size_t plots_bytes(const sarx_cluster_params* p) { return (size_t)p->max_detections * sizeof(sarx_cluster_plot); }

int sarx_cluster_plots_bytes(const sarx_cluster_params* p, size_t* out) {
    return size_query(out, [&] { return cluster_check(nullptr, p); }, [&] { return plots_bytes(p); });
}

// n_frames >= 1; the strides are checked by the caller
static int cluster_run(sarx_ctx* c, const sarx_cluster_params* p, const void* d_in, size_t in_stride, void* d_out, size_t out_stride,
                       int n_frames, void* d_plots, size_t plots_stride, int32_t* d_labels) {
    const DevBuf bufs[] = {need(d_in, 8), need(d_out, 8), opt(d_plots, 8), opt(d_labels, 4)};
    if (const int rc = buffers_ok(c, bufs, "misaligned slot, plot records (8-byte alignment) or labels (4-byte alignment)")) return rc;
    const size_t slot = gmti_slot_bytes(p->max_detections);
    const size_t last = (size_t)(n_frames - 1);
    // in, out and side: the strided extents over all frames; a lone frame's side outputs are held against its output slot as well
    const Span in[] = {{d_in, last * in_stride + slot}}, out[] = {{d_out, last * out_stride + slot}};
    const Span side[] = {{d_plots, last * plots_stride + plots_bytes(p)}, {d_labels, (size_t)n_frames * p->max_detections * sizeof(int32_t)}};
    if (const int rc = check_spans(c, in, out, "cluster input and output slots overlap", nullptr)) return rc;
    if (const int rc = check_spans(c, in, side, "cluster plot records or labels overlap the input", nullptr)) return rc;
    if (n_frames == 1)
        if (const int rc = check_spans(c, out, side, "cluster plot records or labels overlap the output slot", nullptr)) return rc;
    ClusterArgs a{};
    a.p = *p;
    a.in = (const char*)d_in;
    a.out = (char*)d_out;
    a.plots = (char*)d_plots;
    a.labels = d_labels;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.plots_stride = plots_stride;
    HIPCHK(c, launch_cluster(a, n_frames, c->stream));
    return SARX_OK;
}

int sarx_cluster_step_dev(sarx_ctx* c, const sarx_cluster_params* p, const void* d_slot_in, void* d_slot_out, void* d_plots,
                          int32_t* d_labels) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = cluster_check(c, p)) return rc;
        return cluster_run(c, p, d_slot_in, 0, d_slot_out, 0, 1, d_plots, 0, d_labels);
    });
}

int sarx_cluster_run_dev(sarx_ctx* c, const sarx_cluster_params* p, const void* d_in, size_t in_stride_bytes, void* d_out,
                         size_t out_stride_bytes, int n_frames, void* d_plots, size_t plots_stride_bytes, int32_t* d_labels) {
    NEED_CTX(c);
    return guarded(c, [&] {
        if (const int rc = cluster_check(c, p)) return rc;
        if (n_frames < 0) return fail(c, SARX_ERR_INVALID, "cluster n_frames must be >= 0");
        const size_t slot = gmti_slot_bytes(p->max_detections), rec = plots_bytes(p);
        if (!stride_ok(in_stride_bytes, slot) || !stride_ok(out_stride_bytes, slot))
            return fail(c, SARX_ERR_INVALID, "cluster slot strides %zu, %zu must be multiples of 8 and at least the slot's %zu bytes",
                        in_stride_bytes, out_stride_bytes, slot);
        if (d_plots && !stride_ok(plots_stride_bytes, rec))
            return fail(c, SARX_ERR_INVALID, "cluster plot stride %zu must be a multiple of 8 and at least %zu bytes", plots_stride_bytes, rec);
        if (n_frames == 0) return buffers_present(c, {need(d_in, 8), need(d_out, 8)});
        return cluster_run(c, p, d_in, in_stride_bytes, d_out, out_stride_bytes, n_frames, d_plots, plots_stride_bytes, d_labels);
    });
}

}  // extern "C"
