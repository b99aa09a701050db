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
from ._ffi import SarxError, check

HEADER_BYTES = C.sizeof(_ffi.GmtiHeader)
REPORT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("power", "<f8"), ("mean", "<f8"), ("interf_re", "<f8"),
                         ("interf_im", "<f8"), ("mag1", "<f4"), ("mag2", "<f4")])
DETECTION_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("range_m", "<f8"), ("cross_range_m", "<f8"), ("power", "<f8"),
                            ("mean", "<f8"), ("snr_db", "<f8"), ("interf", "<c16"), ("ati_phase", "<f8"), ("v_los_mps", "<f8"),
                            ("cross_range_relocated_m", "<f8"), ("mag1", "<f4"), ("mag2", "<f4")])
assert REPORT_DTYPE.itemsize == C.sizeof(_ffi.GmtiReport) == 48


class GmtiOverflowError(SarxError):
    """More cells qualified than the report list holds: the list is never returned truncated."""

    def __init__(self, count, max_detections):
        super().__init__(-1, f"GMTI: {count} cells qualify, more than max_detections={max_detections}")
        self.count, self.max_detections = int(count), int(max_detections)


def n_full(guard, train):
    """Training cells of a window that lies wholly inside the image."""
    (ga, gr), (ta, tr) = guard, train
    return (2 * (ga + ta) + 1) * (2 * (gr + tr) + 1) - (2 * ga + 1) * (2 * gr + 1)


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
        ga, gr = (int(x) for x in self.guard)
        ta, tr = (int(x) for x in self.train)
        if min(ga, gr, ta, tr) < 0:
            raise ValueError("guard and train half-widths must be >= 0")
        if ga + ta > _ffi.GMTI_MAX_HALF or gr + tr > _ffi.GMTI_MAX_HALF:
            raise ValueError(f"guard + train half-widths ({ga + ta}, {gr + tr}) exceed {_ffi.GMTI_MAX_HALF}")
        nf = n_full((ga, gr), (ta, tr))
        if nf < 1:
            raise ValueError("the training set is empty")
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
        """Bytes of one device slot: header + max_detections reports (sarx_gmti_slot_bytes)."""
        cp = self._base_params()
        n = C.c_size_t()
        lib = _ffi.load()
        check(lib.sarx_gmti_slot_bytes(C.byref(cp), C.byref(n)))
        return n.value


class GmtiReport:
    """Result of a detection: `detections` (structured array, DETECTION_DTYPE, sorted by (i, j)), `n_found`, the `alpha` used, the
    unambiguous radial speed `v_ambiguity_mps` = lambda / (4 lag), the `method` ("ca" / "os") and, for "os", the `rank` (else
    None).  With "os" the `mean` field is the ordered statistic x_(rank), so `snr_db` is power over that level."""

    def __init__(self, detections, alpha, v_ambiguity_mps, n_full_cells, method="ca", rank=None):
        self.detections = detections
        self.n_found = int(len(detections))
        self.alpha = float(alpha)
        self.v_ambiguity_mps = float(v_ambiguity_mps)
        self.n_full = int(n_full_cells)
        self.method = method
        self.rank = None if rank is None else int(rank)
        self.plots = None                    # gmti_detect(cluster=...): the GmtiPlots of this list
        self.gate = None                     # gmti_detect(ati_gate=...): the statistics of every report that went into the gate

    def __len__(self):
        return self.n_found

    def __repr__(self):
        return f"GmtiReport(n_found={self.n_found}, alpha={self.alpha:.4g}, v_ambiguity_mps={self.v_ambiguity_mps:.4g})"


class _Ptr:
    def __init__(self, ptr):
        self.ptr = ptr


def enqueue(ctx, d_mag, d_slc1, d_slc2, n_az, n_rg, params, cal_phase, slot_ptr):
    """CFAR + refine launches on the ctx's current lane into the slot at slot_ptr (header, then the report list).  Device
    pointers, [n_az x n_rg] row-major; only enqueues."""
    cp = params.c_params()
    launch = ctx.lib.sarx_gmti_cfar_dev if params.method == "ca" else ctx.lib.sarx_gmti_oscfar_dev
    check(launch(ctx.h, d_mag, int(n_az), int(n_rg), C.byref(cp), slot_ptr + HEADER_BYTES, slot_ptr), ctx.h)
    check(ctx.lib.sarx_gmti_refine_dev(ctx.h, d_slc1, d_slc2, int(n_az), int(n_rg), float(cal_phase), slot_ptr + HEADER_BYTES,
                                       slot_ptr, int(params.max_detections)), ctx.h)


def fetch_slot(ctx, slot_ptr, max_detections):
    """Header, then the reports it counts (blocking): the raw bytes of a slot, trimmed to its content."""
    hdr = np.empty(HEADER_BYTES, np.uint8)
    check(ctx.lib.sarx_memcpy_d2h(ctx.h, hdr.ctypes.data, slot_ptr, HEADER_BYTES), ctx.h)
    count = int(hdr.view("<u4")[0])
    n = min(count, int(max_detections))
    raw = np.empty(HEADER_BYTES + n * REPORT_DTYPE.itemsize, np.uint8)
    raw[:HEADER_BYTES] = hdr
    if n:
        check(ctx.lib.sarx_memcpy_d2h(ctx.h, raw[HEADER_BYTES:].ctypes.data, slot_ptr + HEADER_BYTES, n * REPORT_DTYPE.itemsize), ctx.h)
    return raw


def decode_slot(raw, params, range_axis, cross_range, wavelength_m, platform_speed_mps, lag_s):
    """A slot's bytes (header + reports) -> GmtiReport.  Raises GmtiOverflowError when the list overflowed."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    count, overflow = (int(x) for x in raw[:8].view("<u4"))
    if overflow or count > params.max_detections:
        raise GmtiOverflowError(count, params.max_detections)
    rep = raw[HEADER_BYTES:HEADER_BYTES + count * REPORT_DTYPE.itemsize].view(REPORT_DTYPE)
    _, _, _, _, nf, alpha = params.resolved()
    lam, lag = float(wavelength_m), float(lag_s)
    out = np.zeros(count, DETECTION_DTYPE)
    ra, ca = np.asarray(range_axis, dtype=np.float64), np.asarray(cross_range, dtype=np.float64)
    for k in ("i", "j", "power", "mean", "mag1", "mag2"):
        out[k] = rep[k]
    out["range_m"] = ra[rep["j"]]
    out["cross_range_m"] = ca[rep["i"]]
    with np.errstate(divide="ignore"):
        out["snr_db"] = 10.0 * np.log10(rep["power"] / rep["mean"])
    out["interf"] = rep["interf_re"] + 1j * rep["interf_im"]
    out["ati_phase"] = np.angle(out["interf"])
    # slc1 (Rx1[1:]) sees the scene one lag after slc2 (Rx2[:-1]) from the same phase centre: a receding target (v_los > 0) is
    # further away for slc1, so angle(slc1 conj(slc2)) = -4 pi v_los lag / lambda; it is imaged R v_los / V earlier in azimuth
    out["v_los_mps"] = -lam * out["ati_phase"] / (4.0 * math.pi * lag)
    out["cross_range_relocated_m"] = out["cross_range_m"] + out["range_m"] * out["v_los_mps"] / float(platform_speed_mps)
    return GmtiReport(out, alpha, lam / (4.0 * lag), nf, params.method, params.rank())


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
        slot = ctx.alloc(params.slot_bytes())
        temps.append(slot)
        enqueue(ctx, pm, p1, p2, n_az, n_rg, params, cal_phase, slot.ptr)
        md = params.max_detections
        if gate_cp is not None:                              # two launches behind refine; everything after it takes the gated slot
            from . import atigate as gat
            full, slot, gstats = slot, ctx.alloc(params.slot_bytes()), ctx.alloc(gat.stats_bytes(gate_cp))
            temps += [slot, gstats]
            gat.enqueue_step(ctx, gate_cp, p1, p2, n_az, n_rg, full.ptr, slot.ptr, gstats.ptr)
        if cluster_cp is not None:
            from . import cluster as clu
            pslot, prec, plab = ctx.alloc(params.slot_bytes()), ctx.alloc(clu.plots_bytes(cluster_cp)), ctx.alloc(md * 4)
            temps += [pslot, prec, plab]
            clu.enqueue_step(ctx, cluster_cp, slot.ptr, pslot.ptr, prec.ptr, plab.ptr)
        raw = fetch_slot(ctx, slot.ptr, params.max_detections)
        gate = gat.fetch_gate(ctx, full.ptr, gstats.ptr).copy() if gate_cp is not None else None
        if cluster_cp is not None:
            plots = clu.fetch_plots(ctx, pslot.ptr, prec.ptr, plab.ptr, md, in_ptr=slot.ptr, detect=params, range_axis=range_axis,
                                    cross_range=cross_range, wavelength_m=wavelength_m, platform_speed_mps=platform_speed_mps,
                                    lag_s=lag_s)
    finally:
        for b in temps:
            b.release()
    report = decode_slot(raw, params, range_axis, cross_range, wavelength_m, platform_speed_mps, lag_s)
    if cluster_cp is not None:
        report.plots = plots
    report.gate = gate
    return report
