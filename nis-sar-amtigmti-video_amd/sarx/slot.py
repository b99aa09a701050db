"""The GMTI slot on the host.  Every stage of the chain (detector, ATI gate, plot extraction, refocus, tracker) hands the next one a
slot: a 16-byte sarx_gmti_header (count, overflow, two reserved words) followed by max_detections 48-byte sarx_gmti_report
(include/sarx_gmti.h).  This module is the only place in sarx/ that knows that layout.

Overflow rule.  `count` is the number of cells that qualified, `overflow` is set when the list could not hold them, md is the
slot's capacity.  What each reader does with them - every site keeps the condition it was written with:
  raise on overflow or count > md   gmti.decode_slot = decode, refocus.refocus_slot, TwoChannelBatch.plots,
  (raise_if_overflowed, strict)     TwoChannelBatch.refocus, tdbp_pair_search.tdbp_pair_search
  raise on overflow alone           atigate.gmti_ati_gate (the gated slot), cluster.GmtiPlots, cluster.fetch_plots (the plot slot)
  (raise_if_overflowed, not strict)
  clamp to min(count, md)           fetch = gmti.fetch_slot (the header itself is kept as it is), track._slot_ij
  no test, the count as it stands   count_of = cluster.count_of, cluster.fetch_plots (n_reports from the input slot)
  no test, overflow = no records    atigate.fetch_gate (else `count` records)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _ffi
from ._ffi import SarxError, check

HEADER_BYTES = C.sizeof(_ffi.GmtiHeader)
REPORT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("power", "<f8"), ("mean", "<f8"), ("interf_re", "<f8"),
                         ("interf_im", "<f8"), ("mag1", "<f4"), ("mag2", "<f4")])
DETECTION_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("range_m", "<f8"), ("cross_range_m", "<f8"), ("power", "<f8"),
                            ("mean", "<f8"), ("snr_db", "<f8"), ("interf", "<c16"), ("ati_phase", "<f8"), ("v_los_mps", "<f8"),
                            ("cross_range_relocated_m", "<f8"), ("mag1", "<f4"), ("mag2", "<f4")])
assert HEADER_BYTES == 16 and REPORT_DTYPE.itemsize == C.sizeof(_ffi.GmtiReport) == 48


class GmtiOverflowError(SarxError):
    """More cells qualified than the report list holds: the list is never returned truncated."""

    def __init__(self, count, max_detections):
        super().__init__(-1, f"GMTI: {count} cells qualify, more than max_detections={max_detections}")
        self.count, self.max_detections = int(count), int(max_detections)


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


def slot_bytes(max_detections):
    """Bytes of one slot: the header and max_detections reports."""
    return HEADER_BYTES + int(max_detections) * REPORT_DTYPE.itemsize


def _bytes(raw):
    return np.ascontiguousarray(raw).view(np.uint8).reshape(-1)


def header(raw):
    """(count, overflow) of a slot's bytes."""
    return tuple(int(x) for x in _bytes(raw)[:8].view("<u4"))


def reports(raw, count=None):
    """View of the first `count` reports of a slot's bytes (None: as many as the header counts; fewer if the bytes end before)."""
    raw = _bytes(raw)
    count = header(raw)[0] if count is None else count
    return raw[HEADER_BYTES:slot_bytes(count)].view(REPORT_DTYPE)


def raise_if_overflowed(count, overflow, max_detections, strict):
    """GmtiOverflowError when the overflow flag is set or (strict) the count exceeds the capacity: the table above.  -> count"""
    if overflow or (strict and count > max_detections):
        raise GmtiOverflowError(count, max_detections)
    return count


def download(ctx, ptr, nbytes):
    """nbytes from the device address ptr (blocking) as a uint8 array; nothing is copied for none."""
    out = np.empty(int(nbytes), np.uint8)
    if nbytes:
        check(ctx.lib.sarx_memcpy_d2h(ctx.h, out.ctypes.data, ptr, int(nbytes)), ctx.h)
    return out


def fetch_header(ctx, ptr):
    """The header of the device slot at ptr (blocking) as bytes."""
    return download(ctx, ptr, HEADER_BYTES)


def fetch(ctx, slot_ptr, max_detections):
    """Header, then the reports it counts (blocking): the raw bytes of a slot, trimmed to its content."""
    hdr = fetch_header(ctx, slot_ptr)
    n = min(header(hdr)[0], int(max_detections))
    return np.concatenate([hdr, download(ctx, slot_ptr + HEADER_BYTES, n * REPORT_DTYPE.itemsize)])


def encode(report, max_detections):
    """A slot's bytes from a GmtiReport, a REPORT_DTYPE array, or a slot's own bytes (padded to the full size)."""
    raw = np.zeros(slot_bytes(max_detections), np.uint8)
    if isinstance(report, GmtiReport):
        d = report.detections
        rep = np.zeros(len(d), REPORT_DTYPE)
        for k in ("i", "j", "power", "mean", "mag1", "mag2"):
            rep[k] = d[k]
        rep["interf_re"], rep["interf_im"] = d["interf"].real, d["interf"].imag
    else:
        a = np.asarray(report)
        if a.dtype == REPORT_DTYPE:
            rep = a
        else:
            a = _bytes(a)
            if a.size > raw.size or a.size < HEADER_BYTES:
                raise ValueError("a raw slot is a header and at most max_detections reports")
            raw[:a.size] = a
            return raw
    if len(rep) > max_detections:
        raise GmtiOverflowError(len(rep), max_detections)
    raw[:4].view("<u4")[0] = len(rep)
    raw[HEADER_BYTES:HEADER_BYTES + rep.nbytes] = _bytes(rep)
    return raw


def count_of(x):
    """Reports in a GmtiReport, a REPORT_DTYPE array or a slot's bytes (its header's count, as it stands)."""
    if isinstance(x, GmtiReport):
        return len(x.detections)
    a = np.asarray(x)
    return len(a) if a.dtype == REPORT_DTYPE else int(_bytes(a)[:4].view("<u4")[0])


def stage(reports, detect=None, max_detections=None, single=False):
    """The `reports` argument of a public entry point -> (md, stack, on_device).  `reports` is a GmtiReport, a REPORT_DTYPE array, a
    slot's bytes, a device slot (anything with .ptr), or - unless `single` - a list of these.  md is the slots' capacity:
    detect.max_detections, else max_detections, else the longest host list (device slots cannot tell theirs).  stack [n x
    slot_bytes(md)] holds the host items encoded, ready to upload; on_device lists (index, pointer) of the others."""
    items = [reports] if single or not isinstance(reports, (list, tuple)) else list(reports)
    on_device = [(f, x.ptr) for f, x in enumerate(items) if hasattr(x, "ptr")]
    if detect is not None:
        md = int(detect.max_detections)
    elif max_detections is not None:
        md = int(max_detections)
    elif on_device:
        raise ValueError("a device slot needs detect= or max_detections= (its capacity)" if single else
                         "device slots need detect= or max_detections= (their capacity)")
    else:
        md = max([1] + [count_of(x) for x in items])
    stack = np.zeros((len(items), slot_bytes(md)), np.uint8)
    for f, x in enumerate(items):
        if not hasattr(x, "ptr"):
            stack[f] = encode(x, md)
    return md, stack, on_device


def lag_of(detect, prf_hz):
    """The lag between the co-registered channels: detect.lag_s, else one pulse."""
    return detect.lag_s if detect.lag_s is not None else 1.0 / prf_hz


def decode(raw, params, range_axis, cross_range, wavelength_m, platform_speed_mps, lag_s):
    """A slot's bytes (header + reports) -> GmtiReport.  Raises GmtiOverflowError when the list overflowed."""
    count = raise_if_overflowed(*header(raw), params.max_detections, strict=True)
    rep = reports(raw, count)
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
