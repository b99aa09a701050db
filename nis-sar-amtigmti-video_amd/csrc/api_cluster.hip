// libsarx C ABI of include/sarx_cluster.h: parameter checks and the launch of cluster.hip.
#include "../../include/sarx_cluster.h"
#include "api_ctx.h"
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

int sarx_cluster_plots_bytes(const sarx_cluster_params* p, size_t* out) {
    if (!out) return fail(nullptr, SARX_ERR_INVALID, "out_bytes is NULL");
    const int rc = cluster_check(nullptr, p);
    if (rc != SARX_OK) return rc;
    *out = (size_t)p->max_detections * sizeof(sarx_cluster_plot);
    return SARX_OK;
}

// n_frames >= 1; the strides are checked by the caller
static int cluster_run(sarx_ctx* c, const sarx_cluster_params* p, const void* d_in, size_t in_stride, void* d_out, size_t out_stride,
                       int n_frames, void* d_plots, size_t plots_stride, int32_t* d_labels) {
    if (!d_in || !d_out) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_plots & 7) || ((uintptr_t)d_labels & 3))
        return fail(c, SARX_ERR_INVALID, "misaligned slot, plot records (8-byte alignment) or labels (4-byte alignment)");
    const size_t slot = gmti_slot_bytes(p->max_detections);
    const size_t last = (size_t)(n_frames - 1);
    const size_t in_span = last * in_stride + slot, out_span = last * out_stride + slot;
    const size_t plots_span = last * plots_stride + (size_t)p->max_detections * sizeof(sarx_cluster_plot);
    const size_t labels_span = (size_t)n_frames * p->max_detections * sizeof(int32_t);
    if (ranges_overlap(d_in, in_span, d_out, out_span)) return fail(c, SARX_ERR_INVALID, "cluster input and output slots overlap");
    if (ranges_overlap(d_in, in_span, d_plots, plots_span) || ranges_overlap(d_in, in_span, d_labels, labels_span))
        return fail(c, SARX_ERR_INVALID, "cluster plot records or labels overlap the input");
    if (n_frames == 1 && (ranges_overlap(d_out, slot, d_plots, plots_span) || ranges_overlap(d_out, slot, d_labels, labels_span)))
        return fail(c, SARX_ERR_INVALID, "cluster plot records or labels overlap the output slot");
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
        const int rc = cluster_check(c, p);
        if (rc != SARX_OK) return rc;
        return cluster_run(c, p, d_slot_in, 0, d_slot_out, 0, 1, d_plots, 0, d_labels);
    });
}

int sarx_cluster_run_dev(sarx_ctx* c, const sarx_cluster_params* p, const void* d_in, size_t in_stride_bytes, void* d_out,
                         size_t out_stride_bytes, int n_frames, void* d_plots, size_t plots_stride_bytes, int32_t* d_labels) {
    NEED_CTX(c);
    return guarded(c, [&] {
        const int rc = cluster_check(c, p);
        if (rc != SARX_OK) return rc;
        if (n_frames < 0) return fail(c, SARX_ERR_INVALID, "cluster n_frames must be >= 0");
        const size_t slot = gmti_slot_bytes(p->max_detections);
        if (in_stride_bytes < slot || (in_stride_bytes & 7) || out_stride_bytes < slot || (out_stride_bytes & 7))
            return fail(c, SARX_ERR_INVALID, "cluster slot strides %zu, %zu must be multiples of 8 and at least the slot's %zu bytes",
                        in_stride_bytes, out_stride_bytes, slot);
        const size_t rec = (size_t)p->max_detections * sizeof(sarx_cluster_plot);
        if (d_plots && (plots_stride_bytes < rec || (plots_stride_bytes & 7)))
            return fail(c, SARX_ERR_INVALID, "cluster plot stride %zu must be a multiple of 8 and at least %zu bytes", plots_stride_bytes, rec);
        if (n_frames == 0) {
            if (!d_in || !d_out) return fail(c, SARX_ERR_INVALID, "NULL device pointer");
            return (int)SARX_OK;
        }
        return cluster_run(c, p, d_in, in_stride_bytes, d_out, out_stride_bytes, n_frames, d_plots, plots_stride_bytes, d_labels);
    });
}

}  // extern "C"
