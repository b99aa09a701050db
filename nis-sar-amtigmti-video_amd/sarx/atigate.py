"""GMTI ATI gate on the GPU: the second step of the two-step DPCA / ATI detector.  A report is kept only when its interferometric
phase stands out from the phase of the clutter around it (include/sarx_atigate.h, csrc/atigate.hip).

Semantics (the kernels implement them; include/sarx_atigate.h states them step by step):
  Per report at (i, j): over the ring T (outer box inside the image minus the guard box, N cells) c11 = sum |a|^2, c22 = sum |b|^2,
  c12 = sum a conj(b) for a = slc1, b = slc2; over the look box (inside the guard box, n_look cells) I = sum a conj(b); all fp64
  sums of exact products.  Untested: N < min_train (reason 1), c11 c22 == 0 or I == 0 (2), coh = |c12| / sqrt(c11 c22) < min_coh
  (3).  Otherwise psi = angle(I conj(c12)) - the report's phase against the local clutter phase - and
  sigma = sqrt((1 - coh^2) / (2 n_look coh^2)); the report PASSES when |psi| > k_sigma sigma and |psi| >= phase_min.  Kept: passed,
  or untested with keep_untested.  The kept reports are byte-for-byte copies in a GMTI slot like the detector's, sorted by (i, j):
  cluster, refocus, tracker and decode_slot take it unchanged.  An overflowing input list stays an overflow: GmtiOverflowError.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _ffi, gmti, slot as _slot
from ._ffi import check
from .slot import slot_bytes   # noqa: F401

GATE_DTYPE = np.dtype([("c11", "<f8"), ("c22", "<f8"), ("c12_re", "<f8"), ("c12_im", "<f8"), ("i_re", "<f8"), ("i_im", "<f8"),
                       ("coh", "<f8"), ("psi", "<f8"), ("sigma", "<f8"), ("n_train", "<i4"), ("n_look", "<i4"), ("status", "<i4"),
                       ("reason", "<i4"), ("out_index", "<i4"), ("reserved", "<i4")])
assert GATE_DTYPE.itemsize == C.sizeof(_ffi.AtiGateStat) == 96
UNTESTED, REJECTED, PASSED = 0, 1, 2


@dataclass
class AtiGateParams:
    """guard, train, looks: (azimuth, range) half-widths of the guard box, the training ring around it and the look box inside it
    (guard + train <= 32, looks 0 .. 4 and <= guard); k_sigma: threshold in Cramer-Rao spreads of the clutter's interferometric
    phase; phase_min: least |psi| of a mover (rad); min_coh: clutter coherence below which a report is untested; min_train: ring
    cells a test needs (None = (N_full + 1) // 2); keep_untested: untested reports stay in the list."""
    guard: Tuple[int, int] = (2, 2)
    train: Tuple[int, int] = (8, 8)
    looks: Tuple[int, int] = (1, 1)
    k_sigma: float = 3.0
    phase_min: float = 0.0
    min_coh: float = 0.3
    min_train: Optional[int] = None
    keep_untested: bool = True

    def check(self):
        try:
            (ga, gr), (ta, tr), (la, lr) = ((int(x) for x in v) for v in (self.guard, self.train, self.looks))
        except (TypeError, ValueError):
            raise ValueError("guard, train and looks must be (azimuth, range) pairs") from None
        *_, nf = gmti.window((ga, gr), (ta, tr))
        if not (0 <= la <= _ffi.ATIGATE_MAX_LOOK and 0 <= lr <= _ffi.ATIGATE_MAX_LOOK):
            raise ValueError(f"looks must lie in 0 .. {_ffi.ATIGATE_MAX_LOOK}")
        if la > ga or lr > gr:
            raise ValueError("the look box must lie inside the guard box (looks <= guard)")
        k, pm, mc = float(self.k_sigma), float(self.phase_min), float(self.min_coh)
        if not (math.isfinite(k) and k >= 0.0):
            raise ValueError("k_sigma must be finite and >= 0")
        if not 0.0 <= pm <= math.pi:
            raise ValueError("phase_min must lie in 0 .. pi")
        if not 0.0 <= mc <= 1.0:
            raise ValueError("min_coh must lie in 0 .. 1")
        mt = (nf + 1) // 2 if self.min_train is None else int(self.min_train)
        if mt < 1:
            raise ValueError("min_train must be >= 1")
        return ga, gr, ta, tr, la, lr, k, pm, mc, mt

    def c_params(self, max_detections):
        ga, gr, ta, tr, la, lr, k, pm, mc, mt = self.check()
        if not 1 <= int(max_detections) <= _ffi.ATIGATE_MAX_DETECTIONS:
            raise ValueError(f"the ATI gate takes report lists of 1 .. {_ffi.ATIGATE_MAX_DETECTIONS} reports (max_detections)")
        return _ffi.AtiGateParams(ga, gr, ta, tr, la, lr, k, pm, mc, mt, int(max_detections),
                                  _ffi.ATIGATE_KEEP_UNTESTED if self.keep_untested else 0, 0)


def stats_bytes(cp):
    n = C.c_size_t()
    check(_ffi.load().sarx_atigate_stats_bytes(C.byref(cp), C.byref(n)))
    return n.value


def enqueue_step(ctx, cp, d_slc1, d_slc2, n_az, n_rg, in_ptr, out_ptr, stats_ptr):
    """The two launches of one frame on the ctx's current lane; only enqueues."""
    check(ctx.lib.sarx_atigate_step_dev(ctx.h, C.byref(cp), d_slc1, d_slc2, int(n_az), int(n_rg), in_ptr, out_ptr, stats_ptr), ctx.h)


def fetch_gate(ctx, in_ptr, stats_ptr):
    """The statistics of the reports the input slot at in_ptr counts (blocking) -> GATE_DTYPE array; empty when it overflowed."""
    count, overflow = _slot.header(_slot.fetch_header(ctx, in_ptr))
    return _slot.download(ctx, stats_ptr, 0 if overflow else count * GATE_DTYPE.itemsize).view(GATE_DTYPE)


def gmti_ati_gate(reports, slc1, slc2, params=None, *, range_axis=None, cross_range=None, wavelength_m=None, platform_speed_mps=None,
                  lag_s=None, detect=None, max_detections=None, shape=None, ctx=None):
    """Keep the reports whose ATI phase stands out from the clutter around them.

    reports : a GmtiReport (gmti_detect, TwoChannelBatch.detections), an array of gmti.REPORT_DTYPE, the raw bytes of a slot, or a
              device slot (anything with .ptr, max_detections reports long)
    slc1, slc2 : the two images, as sarx.gmti_detect takes them: [N_rg x N_az] complex host arrays or [N_az x N_rg] device images
    params  : AtiGateParams
    range_axis, cross_range : the focuser's axes; they give the image size (else shape=(n_az, n_rg)) and, with detect,
              wavelength_m, platform_speed_mps and lag_s, let the gated list be decoded by gmti.decode_slot
    detect  : the detector's GmtiParams: its max_detections is the slots' capacity (else max_detections, else the list's length)
    Returns (gated, gate): `gated` a GmtiReport when it can be decoded, else the kept reports as an array of gmti.REPORT_DTYPE;
    `gate` one GATE_DTYPE record per input report.  Raises GmtiOverflowError for an overflowing input list."""
    from .engine import default_context
    params = params or AtiGateParams()
    md, stack, on_device = _slot.stage(reports, detect, max_detections, single=True)
    cp = params.c_params(md)
    if range_axis is not None and cross_range is not None:
        n_az, n_rg = len(cross_range), len(range_axis)
    elif shape is not None:
        n_az, n_rg = (int(x) for x in shape)
    else:
        a = np.asarray(slc1) if not hasattr(slc1, "ptr") else None
        if a is None:
            raise ValueError("device images need the axes or shape=(n_az, n_rg)")
        n_rg, n_az = a.shape
    ctx = ctx or getattr(slc1, "ctx", None) or default_context()
    temps = []
    try:
        p1 = gmti._plane_ptr(ctx, slc1, n_az, n_rg, np.complex64, temps)
        p2 = gmti._plane_ptr(ctx, slc2, n_az, n_rg, np.complex64, temps)
        if on_device:
            in_ptr = on_device[0][1]
        else:
            temps.append(ctx.to_device(stack[0]))
            in_ptr = temps[-1].ptr
        d_out, d_stats = ctx.alloc(slot_bytes(md)), ctx.alloc(stats_bytes(cp))
        temps += [d_out, d_stats]
        enqueue_step(ctx, cp, p1, p2, n_az, n_rg, in_ptr, d_out.ptr, d_stats.ptr)
        raw = _slot.fetch(ctx, d_out.ptr, md)
        _slot.raise_if_overflowed(*_slot.header(raw), md, strict=False)
        gate = fetch_gate(ctx, in_ptr, d_stats.ptr).copy()
    finally:
        for b in temps:
            b.release()
    if range_axis is not None and cross_range is not None and None not in (detect, wavelength_m, platform_speed_mps, lag_s):
        gated = _slot.decode(raw, detect, range_axis, cross_range, wavelength_m, platform_speed_mps, lag_s)
        gated.gate = gate
    else:
        gated = _slot.reports(raw).copy()
    return gated, gate
