/* libsarx GMTI plot extraction: the reports of one object merged into one plot, on the device.
 *
 * Plain C99.  Extends include/sarx.h and include/sarx_gmti.h (the context, the error codes and the slot layout come from there).
 *
 * Input: a GMTI slot, one sarx_gmti_header followed by max_detections sarx_gmti_report exactly as sarx_gmti_refine_dev leaves it:
 * count n read from the device header, reports sorted by (i, j), no cell twice.  No entry point synchronises with the host, no
 * kernel uses a global atomic, and every output is the same bits from run to run and between sarx_cluster_run_dev and the loop of
 * sarx_cluster_step_dev it stands for.  A list that is not sorted or holds a cell twice gives an unspecified result, but the launch
 * ends and reads and writes nothing outside its buffers.
 *
 * Output: a slot of the same layout that holds the plot list (sorted by (i, j), so sarx_refocus_dev, sarx_track_step_dev and every
 * decoder of a GMTI slot take it unchanged), one sarx_cluster_plot per plot, and one label per input report.
 *
 *    1. overflow     : the input header's overflow flag set or count > max_detections: the output header becomes
 *                      {count, 1, 0, 0}, every label -1, nothing else is written.  A truncated list is never clustered.
 *    2. link         : reports r and s are linked when |i_r - i_s| <= link_az and |j_r - j_s| <= link_rg.  Plots are the connected
 *                      components of that relation (single linkage, transitive).
 *    3. per component, members m_0 < m_1 < ... in rising report index:
 *                      n_members;  peak = the member of largest power (ties: the smaller index; a power is larger when `>` says
 *                      so, starting from m_0);  i_min, i_max, j_min, j_max;
 *                      sum_power = power(m_0) + power(m_1) + ..., sum_re, sum_im likewise over interf_re, interf_im;
 *                      wi = power(m_0) i(m_0) + power(m_1) i(m_1) + ..., wj likewise with j.  All in fp64, the sum of one member is
 *                      that member's value, one addition after another in rising member index, every product rounded on its own
 *                      (no fused multiply-add);
 *                      centroid_i = wi / sum_power, centroid_j = wj / sum_power; the peak's i and j when sum_power == 0;
 *                      max_ratio = the largest power / mean of the members (ratio > max_ratio ? ratio : max_ratio, from m_0's).
 *    4. keep         : a component with n_members >= min_members.
 *    5. order        : the kept plots in rising report index of their peak, so the plot list is sorted by (i, j).
 *    6. plot k       : output report k = the peak's report with interf_re, interf_im replaced by sum_re, sum_im;
 *                      plots[k] = the sarx_cluster_plot below;  labels[r] = k for its members.  Members of a dropped component get
 *                      label -1.  All max_detections labels are written, -1 past n.
 *    7. header       : {n_plots, 0, 0, 0}.  Output reports and plot records past n_plots are not touched.
 *    8. consequences : with link = (0, 0) and min_members = 1 the first 16 + 48 n bytes of the output slot equal the input's (a
 *                      header whose reserved words are 0) and labels[r] = r;  n_plots <= n, so the output never overflows.
 *
 * Left out: growing regions over the DPCA plane itself (the CFAR keeps nothing per cell), linkage in relocated ground coordinates,
 * and a parallel reduction inside one plot (each plot is summed by one thread). */
#ifndef SARX_CLUSTER_H
#define SARX_CLUSTER_H

#include "sarx.h"
#include "sarx_gmti.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SARX_CLUSTER_MAX_LINK 64
#define SARX_CLUSTER_MAX_DETECTIONS 16384

typedef struct {
    int32_t link_az, link_rg;      /* link half-widths in pixels, 0 .. SARX_CLUSTER_MAX_LINK */
    int32_t min_members;           /* >= 1 */
    int32_t max_detections;        /* capacity of both slots, 1 .. SARX_CLUSTER_MAX_DETECTIONS */
} sarx_cluster_params;             /* 16 bytes */

typedef struct {
    int32_t n_members;
    int32_t peak_report;           /* index of the peak in the INPUT list */
    int32_t i_min, i_max, j_min, j_max;
    double sum_power;
    double centroid_i, centroid_j; /* power-weighted, pixels */
    double max_ratio;              /* largest power / mean among the members */
    uint32_t reserved[2];          /* 0 */
} sarx_cluster_plot;               /* 64 bytes */

/* validates the parameters (no device needed) */
int sarx_cluster_check(const sarx_cluster_params* params);
/* bytes of the plot records of one frame (max_detections sarx_cluster_plot) */
int sarx_cluster_plots_bytes(const sarx_cluster_params* params, size_t* out_bytes);
/* one frame: the slot at d_slot_in into the slot at d_slot_out (both 8-byte aligned, sarx_gmti_slot_bytes long; they must not
 * overlap, nor may d_plots or d_labels overlap either of them: SARX_ERR_INVALID).  d_plots: max_detections sarx_cluster_plot (8-byte
 * aligned) or NULL; d_labels: max_detections int32 (4-byte aligned) or NULL.  One launch on the ctx's current lane. */
int sarx_cluster_step_dev(sarx_ctx* ctx, const sarx_cluster_params* params, const void* d_slot_in, void* d_slot_out, void* d_plots,
                          int32_t* d_labels);
/* n_frames frames in ONE launch: frame f reads d_in + f in_stride_bytes, writes d_out + f out_stride_bytes and (d_plots not NULL)
 * d_plots + f plots_stride_bytes.  The slot strides are multiples of 8 and at least the slot's size (records behind the reports are
 * skipped), the plot stride a multiple of 8 and at least sarx_cluster_plots_bytes.  The input stack and the output stack must not
 * overlap.  d_labels: [n_frames x max_detections] int32 or NULL.  Only enqueues, on the ctx's current lane. */
int sarx_cluster_run_dev(sarx_ctx* ctx, const sarx_cluster_params* params, const void* d_in, size_t in_stride_bytes, void* d_out,
                         size_t out_stride_bytes, int n_frames, void* d_plots, size_t plots_stride_bytes, int32_t* d_labels);

#ifdef __cplusplus
}
#endif
#endif /* SARX_CLUSTER_H */
