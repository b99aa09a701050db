"""GMTI detection on the GPU: cell-averaging CFAR on the DPCA magnitude plane, each peak refined with the ATI interferogram of
its 3 x 3 neighbourhood and turned into a radial velocity and a relocated azimuth position (include/sarx_gmti.h, csrc/gmti.hip).

Semantics (the kernels implement them; the host only derives the fields from the device's reports):
  P = m^2 in fp64 for the DPCA magnitude m[i, j] ([n_az x n_rg], i = azimuth).  Guard box |di| <= ga, |dj| <= gr; outer box
  |di| <= ga + ta, |dj| <= gr + tr (each at most 32).  The training set T is the outer box inside the image minus the guard box,
  N = |T|; a cell is tested when N >= N_full / 2 and detected when P > alpha * mean_T(P), alpha = N_full (pfa^(-1/N_full) - 1) -
  edge cells with a smaller N keep that full-window alpha.  A detected cell is reported when its P is the maximum over its guard
  box (ties: the smaller linear index).  Reports come sorted by (i, j); more than max_detections of them raise.

method="os" (include/sarx_oscfar.h, csrc/oscfar.hip) replaces the mean by an ordered statistic: with k = ceil(rank N / N_full) a
cell is detected when P > 0 and at least k of its training cells have alpha * P_t < P, i.e. when P > alpha * x_(k) for the k-th
smallest training power x_(k).  alpha = os_cfar_alpha(pfa, N_full, rank); edge cells keep that full-window alpha, as in CA.  The
report's `mean` is then x_(k), the level the cell was held against.  Everything else - peak rule, slot, refine - is shared.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from ._ffi import check
from .batch import _Ptr
# the slot's layout, its errors and its decoded form live in slot.py; these names stay importable from here
from .slot import (DETECTION_DTYPE, HEADER_BYTES, REPORT_DTYPE, GmtiOverflowError, GmtiReport, decode as decode_slot,   # noqa: F401
                   fetch as fetch_slot, lag_of, slot_bytes)


def n_full(guard, train):
    """Training cells of a window that lies wholly inside the image."""
    (ga, gr), (ta, tr) = guard, train
    return (2 * (ga + ta) + 1) * (2 * (gr + tr) + 1) - (2 * ga + 1) * (2 * gr + 1)


def window(guard, train):
    """The (azimuth, range) half-widths of a guard box and the training ring around it, checked -> ga, gr, ta, tr, N_full."""
    (ga, gr), (ta, tr) = ((int(x) for x in v) for v in (guard, train))
    if min(ga, gr, ta, tr) < 0:
        raise ValueError("guard and train half-widths must be >= 0")
    if ga + ta > _ffi.GMTI_MAX_HALF or gr + tr > _ffi.GMTI_MAX_HALF:
        raise ValueError(f"guard + train half-widths ({ga + ta}, {gr + tr}) exceed {_ffi.GMTI_MAX_HALF}")
    nf = n_full((ga, gr), (ta, tr))
    if nf < 1:
        raise ValueError("the training set is empty")
    return ga, gr, ta, tr, nf


def cfar_alpha(pfa, n):
    """CA-CFAR threshold factor for exponentially distributed power: alpha = N (pfa^(-1/N) - 1)."""
    if not (0.0 < pfa < 1.0) or n < 1:
        raise ValueError("pfa must lie in (0, 1) and the training set must not be empty")
    return n * (pfa ** (-1.0 / n) - 1.0)


def _os_log_pfa(alpha, n, rank):
    return -math.fsum(math.log1p(alpha / (n - i)) for i in range(rank))


def os_cfar_pfa(alpha, n, rank):
    """False-alarm rate of OS-CFAR on exponentially distributed power: prod_{i < rank} (n - i) / (n - i + alpha), in logs."""
    return math.exp(_os_log_pfa(alpha, n, rank))


def os_cfar_alpha(pfa, n, rank):
    """OS-CFAR threshold factor for exponentially distributed power: the alpha at which os_cfar_pfa(alpha, n, rank) = pfa, by
    bisection (the rate falls monotonically with alpha).  n = rank = 1 gives 1 / pfa - 1."""
    if not (0.0 < pfa < 1.0) or n < 1 or not 1 <= rank <= n:
        raise ValueError("pfa must lie in (0, 1) and the rank in 1 .. n")
    want = math.log(pfa)
    lo, hi = 0.0, 1.0
    while _os_log_pfa(hi, n, rank) > want:
        lo, hi = hi, 2.0 * hi
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            return hi
        if _os_log_pfa(mid, n, rank) > want:
            lo = mid
        else:
            hi = mid


METHODS = ("ca", "os")


@dataclass
class GmtiParams:
    """Detector settings: half-widths (azimuth, range), false-alarm rate or alpha, capacity of the report list, the lag
    between the co-registered channels (None = one pulse, 1 / prf), the method ("ca" cell averaging, "os" ordered statistic) and
    the ordered statistic's rank (None = (3 N_full) // 4)."""
    guard: Tuple[int, int] = (2, 2)
    train: Tuple[int, int] = (8, 8)
    pfa: float = 1e-6
    alpha: Optional[float] = None
    max_detections: int = 4096
    lag_s: Optional[float] = None
    method: str = "ca"
    os_rank: Optional[int] = None

    def rank(self):
        """The ordered statistic's rank for method="os" (None for "ca")."""
        if self.method not in METHODS:
            raise ValueError(f"method {self.method!r}: one of {METHODS}")
        if self.method == "ca":
            if self.os_rank is not None:
                raise ValueError('os_rank needs method="os"')
            return None
        nf = n_full(tuple(int(x) for x in self.guard), tuple(int(x) for x in self.train))
        rank = (3 * nf) // 4 if self.os_rank is None else int(self.os_rank)
        if not 1 <= rank <= nf:
            raise ValueError(f"os_rank {rank} must be 1 .. N_full = {nf}")
        return rank

    def resolved(self):
        ga, gr, ta, tr, nf = window(self.guard, self.train)
        rank = self.rank()
        if self.alpha is not None:
            alpha = float(self.alpha)
        else:
            alpha = cfar_alpha(float(self.pfa), nf) if rank is None else os_cfar_alpha(float(self.pfa), nf, rank)
        if not (alpha > 0.0 and math.isfinite(alpha)):
            raise ValueError("alpha must be finite and > 0")
        if int(self.max_detections) < 1:
            raise ValueError("max_detections must be >= 1")
        return ga, gr, ta, tr, nf, alpha

    def _base_params(self):
        ga, gr, ta, tr, nf, alpha = self.resolved()
        return _ffi.GmtiParams(ga, gr, ta, tr, alpha, (nf + 1) // 2, int(self.max_detections))

    def c_params(self):
        """sarx_gmti_params for method="ca", sarx_oscfar_params for method="os"."""
        base = self._base_params()
        return base if self.method == "ca" else _ffi.OscfarParams(base, self.rank(), 0)

    def slot_bytes(self):
        """Bytes of one device slot: header + max_detections reports (what sarx_gmti_slot_bytes answers)."""
        self.resolved()
        return slot_bytes(self.max_detections)


def enqueue(ctx, d_mag, d_slc1, d_slc2, n_az, n_rg, params, cal_phase, slot_ptr):
    """CFAR + refine launches on the ctx's current lane into the slot at slot_ptr (header, then the report list).  Device
    pointers, [n_az x n_rg] row-major; only enqueues."""
    cp = params.c_params()
    launch = ctx.lib.sarx_gmti_cfar_dev if params.method == "ca" else ctx.lib.sarx_gmti_oscfar_dev
    check(launch(ctx.h, d_mag, int(n_az), int(n_rg), C.byref(cp), slot_ptr + HEADER_BYTES, slot_ptr), ctx.h)
    check(ctx.lib.sarx_gmti_refine_dev(ctx.h, d_slc1, d_slc2, int(n_az), int(n_rg), float(cal_phase), slot_ptr + HEADER_BYTES,
                                       slot_ptr, int(params.max_detections)), ctx.h)


def enqueue_chain(ctx, d_mag, d_slc1, d_slc2, n_az, n_rg, params, cal_phase, slots, gate=None, cluster=None):
    """The chain in its fixed order on the ctx's current lane: detect (CFAR or OS-CFAR, refine), the ATI gate when `gate` =
    (its c_params, statistics pointer or None) is given, the plot extraction when `cluster` = (its c_params, plot records pointer,
    labels pointer or None) is given.  `slots`: one slot pointer per stage that runs, in that order - every stage reads the slot of
    the stage before it and writes its own.  Returns the last slot written, the one refocus, tracker or fetch read next.  The caller
    owns every buffer; only enqueues."""
    from . import atigate, cluster as clu
    slots = iter(slots)
    cur = next(slots)
    enqueue(ctx, d_mag, d_slc1, d_slc2, n_az, n_rg, params, cal_phase, cur)
    if gate is not None:
        src, cur = cur, next(slots)
        atigate.enqueue_step(ctx, gate[0], d_slc1, d_slc2, n_az, n_rg, src, cur, gate[1])
    if cluster is not None:
        src, cur = cur, next(slots)
        clu.enqueue_step(ctx, cluster[0], src, cur, cluster[1], cluster[2])
    return cur


def run_chain(ctx, d_mag, d_slc1, d_slc2, n_az, n_rg, cal_phase, gate_cp, cluster_cp, decode, then=None):
    """The chain for a caller that keeps no slots (gmti_detect, focus_ati_dpca): temporaries for every stage (a slot each, the gate's
    statistics, the plot records and labels), enqueue_chain, `then`(the last slot's pointer) while they live - focus_ati_dpca's
    refocus -, and the downloads (blocking).  decode: decode_slot's arguments after raw.  Returns the GmtiReport of the detector's
    list - with a gate the gated one, the statistics as its .gate -, the GmtiPlots or None, and what `then` returned."""
    from . import atigate, cluster as clu
    params, held = decode[0], []
    md, size = params.max_detections, params.slot_bytes()

    def alloc(nbytes):
        held.append(ctx.alloc(nbytes))
        return held[-1].ptr
    try:
        slots, gate, cluster, stats, plots = [alloc(size)], None, None, None, None
        if gate_cp is not None:
            slots.append(alloc(size))
            gate = (gate_cp, alloc(atigate.stats_bytes(gate_cp)))
        if cluster_cp is not None:
            slots.append(alloc(size))
            cluster = (cluster_cp, alloc(clu.plots_bytes(cluster_cp)), alloc(md * 4))
        last = enqueue_chain(ctx, d_mag, d_slc1, d_slc2, n_az, n_rg, params, cal_phase, slots, gate, cluster)
        extra = then(last) if then else None
        out = slots[0] if gate is None else slots[1]
        raw = fetch_slot(ctx, out, md)
        if gate is not None:
            stats = atigate.fetch_gate(ctx, slots[0], gate[1]).copy()
        if cluster is not None:
            plots = clu.fetch_plots(ctx, last, cluster[1], cluster[2], md, in_ptr=out, decode=decode)
    finally:
        for b in held:
            b.release()
    report = decode_slot(raw, *decode)
    report.gate = stats
    return report, plots, extra


def _plane_ptr(ctx, x, n_az, n_rg, dtype, temps):
    """Device address of an [n_az x n_rg] row-major plane given as a DeviceArray (or its .T), a DeviceBuffer of that layout, or a
    host [N_rg x N_az] array (the view sar_focus_csa returns), uploaded into a temporary buffer."""
    from .engine import DeviceArray, DeviceBuffer
    item = np.dtype(dtype).itemsize
    if isinstance(x, DeviceArray):
        mem = x.shape[::-1] if x.transposed else x.shape
        if mem != (n_az, n_rg) or item != 8:
            raise ValueError(f"device image of shape {mem} (row-major), expected ({n_az}, {n_rg}) complex64")
        return x.ptr
    if isinstance(x, (DeviceBuffer, _Ptr)):
        if isinstance(x, DeviceBuffer) and x.nbytes < n_az * n_rg * item:
            raise ValueError("device buffer smaller than the plane")
        return x.ptr
    a = np.asarray(x)
    if a.shape != (n_rg, n_az):
        raise ValueError(f"host arrays are [N_rg x N_az] = ({n_rg}, {n_az}) like sar_focus_csa's result, got {a.shape}")
    b = ctx.to_device(np.ascontiguousarray(a.T, dtype=dtype))
    temps.append(b)
    return b.ptr


def gmti_detect(slc1, slc2, range_axis, cross_range, *, wavelength_m, platform_speed_mps, lag_s, guard=(2, 2), train=(8, 8),
                pfa=1e-6, alpha=None, cal_phase=0.0, max_detections=4096, dpca_mag=None, ctx=None, method="ca", os_rank=None, cluster=None, ati_gate=None):
    """Detect movers in a focused two-channel pair and measure their radial speed.

    slc1, slc2  : [N_rg x N_az] complex host arrays (sar_focus_csa's views), or device images ([N_az x N_rg] DeviceArray /
                  DeviceBuffer, e.g. focus_ati_dpca(device_output=True))
    range_axis, cross_range : the focuser's axes (N_rg, N_az)
    lag_s       : time between the co-registered channels (1 / prf for the DPCA pulse shift)
    dpca_mag    : the DPCA magnitude plane (same layouts, fp32); None = computed here by the ATI/DPCA launch with cal_phase
    method      : "ca" (cell averaging) or "os" (ordered statistic of rank os_rank, None = (3 N_full) // 4)
    cluster     : sarx.ClusterParams: the plot extraction (sarx.gmti_cluster) runs on the report list on the device; the
                  GmtiReport returned (the raw report list, as always) then carries the GmtiPlots as `.plots`
    ati_gate    : sarx.AtiGateParams: the ATI gate (sarx.gmti_ati_gate) runs on the report list on the device straight after
                  refine and before `cluster`; the GmtiReport returned is the GATED list and carries the statistics of every
                  report that went in as `.gate` (atigate.GATE_DTYPE)
    Returns a GmtiReport; raises GmtiOverflowError if more than max_detections cells qualify."""
    from .engine import default_context
    params = GmtiParams(tuple(guard), tuple(train), pfa, alpha, int(max_detections), lag_s, method, os_rank)
    params.resolved()
    cluster_cp = cluster.c_params(params.max_detections) if cluster is not None else None
    gate_cp = ati_gate.c_params(params.max_detections) if ati_gate is not None else None
    ctx = ctx or getattr(slc1, "ctx", None) or default_context()
    n_rg, n_az = len(range_axis), len(cross_range)
    n = n_az * n_rg
    temps = []
    try:
        p1 = _plane_ptr(ctx, slc1, n_az, n_rg, np.complex64, temps)
        p2 = _plane_ptr(ctx, slc2, n_az, n_rg, np.complex64, temps)
        if dpca_mag is None:
            outs = {k: ctx.alloc(n * 4) for k in ("ati_phase", "slc1_mag", "dpca_mag")}
            temps += list(outs.values())
            ctx.ati_dpca(_Ptr(p1), _Ptr(p2), n, cal_phase, outs, want_stats=False)
            pm = outs["dpca_mag"].ptr
        else:
            pm = _plane_ptr(ctx, dpca_mag, n_az, n_rg, np.float32, temps)
        report, report.plots, _ = run_chain(ctx, pm, p1, p2, n_az, n_rg, cal_phase, gate_cp, cluster_cp,
                                            (params, range_axis, cross_range, wavelength_m, platform_speed_mps, lag_s))
    finally:
        for b in temps:
            b.release()
    return report
