"""GMTI plot extraction on the GPU: the reports of one object - its range and azimuth sidelobes, its DPCA residue, the separate
scatterers of a ship or a vehicle - merged into ONE plot between the detector and the tracker (include/sarx_cluster.h,
csrc/cluster.hip).

Semantics (the kernel implements them; include/sarx_cluster.h states them step by step):
  Reports r and s are linked when |i_r - i_s| <= link_az and |j_r - j_s| <= link_rg; plots are the connected components (single
  linkage).  A plot keeps the report of its strongest member (ties: the smaller index) with the interferogram replaced by the
  coherent sum over the members - one ATI speed for the whole object - and gets a record with the member count, the extent, the
  summed power, the power-weighted centroid and the largest power / mean.  Components of fewer than min_members reports are
  dropped.  The plot list is a GMTI slot like the detector's, sorted by (i, j): refocus, tracker and decode_slot take it unchanged.
  An overflowing input list stays an overflow: GmtiOverflowError, never a truncated answer.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _ffi, slot as _slot
from ._ffi import check
from .slot import count_of, slot_bytes   # noqa: F401

PLOT_DTYPE = np.dtype([("n_members", "<i4"), ("peak_report", "<i4"), ("i_min", "<i4"), ("i_max", "<i4"), ("j_min", "<i4"),
                       ("j_max", "<i4"), ("sum_power", "<f8"), ("centroid_i", "<f8"), ("centroid_j", "<f8"), ("max_ratio", "<f8"),
                       ("reserved", "<u4", (2,))])
PLOT_AXES_DTYPE = np.dtype(PLOT_DTYPE.descr + [("extent_az_m", "<f8"), ("extent_rg_m", "<f8"), ("centroid_range_m", "<f8"),
                                               ("centroid_cross_range_m", "<f8")])
assert PLOT_DTYPE.itemsize == C.sizeof(_ffi.ClusterPlot) == 64


@dataclass
class ClusterParams:
    """link: (azimuth, range) half-widths in pixels of the box inside which two reports belong together (0 .. 64 each);
    min_members: plots of fewer reports are dropped."""
    link: Tuple[int, int] = (4, 4)
    min_members: int = 1

    def check(self):
        try:
            az, rg = (int(x) for x in self.link)
        except (TypeError, ValueError):
            raise ValueError("link must be (link_az, link_rg)") from None
        if not (0 <= az <= _ffi.CLUSTER_MAX_LINK and 0 <= rg <= _ffi.CLUSTER_MAX_LINK):
            raise ValueError(f"link half-widths must lie in 0 .. {_ffi.CLUSTER_MAX_LINK}")
        if int(self.min_members) < 1:
            raise ValueError("min_members must be >= 1")
        return az, rg

    def c_params(self, max_detections):
        az, rg = self.check()
        if not 1 <= int(max_detections) <= _ffi.CLUSTER_MAX_DETECTIONS:
            raise ValueError(f"clustering takes report lists of 1 .. {_ffi.CLUSTER_MAX_DETECTIONS} reports (max_detections)")
        return _ffi.ClusterParams(az, rg, int(self.min_members), int(max_detections))


def plots_bytes(cp):
    n = C.c_size_t()
    check(_ffi.load().sarx_cluster_plots_bytes(C.byref(cp), C.byref(n)))
    return n.value


def enqueue_step(ctx, cp, in_ptr, out_ptr, plots_ptr, labels_ptr):
    """One frame's launch on the ctx's current lane; only enqueues."""
    check(ctx.lib.sarx_cluster_step_dev(ctx.h, C.byref(cp), in_ptr, out_ptr, plots_ptr, labels_ptr), ctx.h)


def enqueue_run(ctx, cp, in_ptr, in_stride, out_ptr, out_stride, n_frames, plots_ptr, plots_stride, labels_ptr):
    """n_frames frames in one launch, slots `in_stride` / `out_stride` bytes apart; only enqueues."""
    check(ctx.lib.sarx_cluster_run_dev(ctx.h, C.byref(cp), in_ptr, int(in_stride), out_ptr, int(out_stride), int(n_frames), plots_ptr,
                                       int(plots_stride), labels_ptr), ctx.h)


class GmtiPlots:
    """The plots of one frame.  `reports`: the plot list as the device wrote it (gmti.REPORT_DTYPE, sorted by (i, j));
    `detections`: the same list as a GmtiReport from gmti.decode_slot - v_los_mps, snr_db and the relocated position from the summed
    interferogram - when the axes and the radar were given, else None; `plots`: one record per plot (PLOT_DTYPE; with axes
    PLOT_AXES_DTYPE: extent_az_m, extent_rg_m, centroid_range_m, centroid_cross_range_m besides); `labels`: plot index per input
    report, -1 for a dropped one, or None when they were not kept; `n_reports`: reports that went in; `raw`: the plot slot's bytes."""

    def __init__(self, raw, plots_raw, labels, n_reports, detect=None, range_axis=None, cross_range=None, wavelength_m=None,
                 platform_speed_mps=None, lag_s=None):
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        count, overflow = _slot.header(raw)
        _slot.raise_if_overflowed(count, overflow, detect.max_detections if detect is not None else count, strict=False)
        self.raw, self.n_plots, self.n_reports = raw[:slot_bytes(count)], count, int(n_reports)
        self.reports = _slot.reports(self.raw, count)
        rec = np.ascontiguousarray(plots_raw).view(np.uint8).reshape(-1)[:count * PLOT_DTYPE.itemsize].view(PLOT_DTYPE)
        self.labels = None if labels is None else np.asarray(labels, np.int32)[:self.n_reports].copy()
        have_axes = range_axis is not None and cross_range is not None
        if have_axes:
            ra, ca = np.asarray(range_axis, np.float64), np.asarray(cross_range, np.float64)
            p = np.zeros(count, PLOT_AXES_DTYPE)
            for name in PLOT_DTYPE.names:
                p[name] = rec[name]
            p["extent_az_m"] = np.abs(ca[rec["i_max"]] - ca[rec["i_min"]])
            p["extent_rg_m"] = np.abs(ra[rec["j_max"]] - ra[rec["j_min"]])
            p["centroid_range_m"] = np.interp(rec["centroid_j"], np.arange(len(ra)), ra)
            p["centroid_cross_range_m"] = np.interp(rec["centroid_i"], np.arange(len(ca)), ca)
            self.plots = p
        else:
            self.plots = rec.copy()
        self.detections = None
        if have_axes and None not in (detect, wavelength_m, platform_speed_mps, lag_s):
            self.detections = _slot.decode(self.raw, detect, range_axis, cross_range, wavelength_m, platform_speed_mps, lag_s)

    def __len__(self):
        return self.n_plots

    def __repr__(self):
        return f"GmtiPlots({self.n_plots} plots of {self.n_reports} reports)"


def fetch_plots(ctx, out_ptr, plots_ptr, labels_ptr, max_detections, n_reports=None, in_ptr=None, decode=()):
    """Download one frame's plot slot, the records it counts and (labels_ptr not None) its labels (blocking) -> GmtiPlots.
    n_reports is read from the input slot at in_ptr when it is not given; decode: GmtiPlots' arguments after it."""
    raw = _slot.fetch(ctx, out_ptr, max_detections)
    count = _slot.raise_if_overflowed(*_slot.header(raw), max_detections, strict=False)
    if n_reports is None:
        n_reports = _slot.header(_slot.fetch_header(ctx, in_ptr))[0]
    rec = _slot.download(ctx, plots_ptr, count * PLOT_DTYPE.itemsize)
    labels = _slot.download(ctx, labels_ptr, max_detections * 4).view(np.int32) if labels_ptr is not None else None
    return GmtiPlots(raw, rec, labels, n_reports, *decode)


def gmti_cluster(reports, params=None, *, range_axis=None, cross_range=None, wavelength_m=None, platform_speed_mps=None, lag_s=None,
                 detect=None, max_detections=None, ctx=None):
    """Merge the reports of one object into one plot.

    reports : a GmtiReport (gmti_detect, TwoChannelBatch.detections), an array of gmti.REPORT_DTYPE, the raw bytes of a slot, a
              device slot (anything with .ptr, max_detections reports long), or a list of these - the list goes up as one stack and
              is clustered in ONE launch.
    params  : ClusterParams
    detect  : the detector's GmtiParams: its max_detections is the slots' capacity (else max_detections, else the longest list),
              and with range_axis, cross_range, wavelength_m, platform_speed_mps and lag_s the plot list is decoded by
              gmti.decode_slot into GmtiPlots.detections.
    Returns a GmtiPlots, or a list of them for a list; raises GmtiOverflowError for an overflowing input list."""
    from .engine import default_context
    params = params or ClusterParams()
    many = isinstance(reports, (list, tuple))
    md, stack, on_device = _slot.stage(reports, detect, max_detections)
    cp = params.c_params(md)
    ctx = ctx or default_context()
    n, slot, rec = len(stack), slot_bytes(md), plots_bytes(cp)
    if n == 0:
        return []
    decode = (detect, range_axis, cross_range, wavelength_m, platform_speed_mps, lag_s)
    bufs = [ctx.to_device(stack), ctx.alloc(n * slot), ctx.alloc(n * rec), ctx.alloc(n * md * 4)]
    try:
        d_in, d_out, d_plots, d_labels = bufs
        for f, ptr in on_device:
            check(ctx.lib.sarx_memcpy_d2d(ctx.h, d_in.ptr + f * slot, ptr, slot), ctx.h)
        if many:
            enqueue_run(ctx, cp, d_in.ptr, slot, d_out.ptr, slot, n, d_plots.ptr, rec, d_labels.ptr)
        else:
            enqueue_step(ctx, cp, d_in.ptr, d_out.ptr, d_plots.ptr, d_labels.ptr)
        out = [fetch_plots(ctx, d_out.ptr + f * slot, d_plots.ptr + f * rec, d_labels.ptr + f * md * 4, md, in_ptr=d_in.ptr + f * slot,
                           decode=decode) for f in range(n)]
    finally:
        for b in bufs:
            b.release()
    return out if many else out[0]
