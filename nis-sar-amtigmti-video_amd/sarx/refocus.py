"""GMTI refocus on the GPU: an azimuth FM-rate search around each GMTI report that estimates the mover's along-track speed and
sharpens its image (include/sarx_refocus.h, csrc/refocus.hip).

The focuser compresses every pixel with the stationary azimuth filter exp(j 4 pi R D(f; V_r) / lambda).  A target moving along
track at v_a has another effective speed V', so its image is smeared in azimuth.  For each report an L x W chip of the DPCA
difference slc1 - slc2 e^{j cal} (or of slc1) is re-compressed with n_hyp speeds V'_k:
  Y_k = ifft_az(fft_az(x) H_k),  H_k(f, j) = exp(j 4 pi R_j / lambda (D(f; V'_k) - D(f; V_r))),  f = fftfreq(L, 1/prf)
and scored by the sharpness S_k = sum |Y_k|^4 / (sum |x|^2)^2; k* = argmax S_k.  The grid is uniform in along-track speed:
  V'_k = V_r (1 - v_k / V_g),  v_along = V_g (1 - V' / V_r)
with V_g the footprint's ground speed (on the reference orbit R R'' is proportional to (omega - v_a / Re)^2, so
V' / V_r - 1 = -v_a / V_g; the flat, airborne limit is V_g = V_r).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _ffi, slot as _slot
from ._ffi import check
from .gmti import HEADER_BYTES, REPORT_DTYPE, GmtiOverflowError, GmtiReport, _plane_ptr   # noqa: F401

RECORD_DTYPE = np.dtype([("k_best", "<i4"), ("i0", "<i4"), ("peak_i", "<i4"), ("peak_j", "<i4"), ("s_prev", "<f4"), ("s_best", "<f4"),
                         ("s_next", "<f4"), ("s_identity", "<f4"), ("peak_power", "<f4"), ("orig_power", "<f4"), ("reserved", "<i4", (2,))])
RESULT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("k_best", "<i4"), ("v_along_mps", "<f8"), ("v_along_grid_mps", "<f8"),
                         ("at_grid_edge", "?"), ("refocus_gain_db", "<f8"), ("sharpness", "<f8"), ("sharpness_identity", "<f8"),
                         ("sharpness_gain", "<f8"), ("peak_i", "<i4"), ("peak_j", "<i4"), ("i0", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(_ffi.RefocusRecord) == 48
assert C.sizeof(_ffi.RefocusParams) == 576
CHIP_LENGTHS = (64, 128, 256, 512)
SOURCES = {"dpca": _ffi.REFOCUS_DPCA, "slc1": _ffi.REFOCUS_SLC1}


@dataclass
class RefocusParams:
    """Refocus settings: chip (L azimuth rows, W range columns), the along-track speed range searched and its number of
    hypotheses, the chip source ("dpca" or "slc1"), the footprint ground speed V_g that maps V' to along-track speed
    (None = the platform speed V_r: the flat, airborne assumption; on an orbit pass V_sat Re / R_sat), and whether the
    sharpness curves and the refocused chips are returned."""
    chip: Tuple[int, int] = (256, 5)
    v_along: Tuple[float, float] = (-40.0, 40.0)
    n_hyp: int = 33
    source: str = "dpca"
    footprint_speed_mps: Optional[float] = None
    want_curves: bool = False
    want_chips: bool = False

    def validate(self, n_az=None):
        L, W = (int(x) for x in self.chip)
        if L not in CHIP_LENGTHS:
            raise ValueError(f"chip length {L} must be one of {CHIP_LENGTHS}")
        if not (1 <= W <= _ffi.REFOCUS_MAX_W and W % 2 == 1):
            raise ValueError(f"chip width {W} must be odd and 1 .. {_ffi.REFOCUS_MAX_W}")
        if n_az is not None and L > n_az:
            raise ValueError(f"chip length {L} exceeds the {n_az} azimuth rows")
        if not (1 <= int(self.n_hyp) <= _ffi.REFOCUS_MAX_HYP):
            raise ValueError(f"n_hyp {self.n_hyp} must be 1 .. {_ffi.REFOCUS_MAX_HYP}")
        if self.source not in SOURCES:
            raise ValueError(f"source must be one of {tuple(SOURCES)}")
        v0, v1 = (float(x) for x in self.v_along)
        if not (math.isfinite(v0) and math.isfinite(v1) and v0 <= v1):
            raise ValueError("v_along must be a finite (low, high) pair")
        if self.footprint_speed_mps is not None and not (float(self.footprint_speed_mps) > 0.0):
            raise ValueError("footprint_speed_mps must be > 0")
        return L, W

    def v_grid(self):
        """The along-track speeds v_k of the hypotheses (uniform)."""
        return np.linspace(float(self.v_along[0]), float(self.v_along[1]), int(self.n_hyp))

    def ground_speed(self, platform_speed_mps):
        return float(self.footprint_speed_mps) if self.footprint_speed_mps is not None else float(platform_speed_mps)

    def speeds(self, platform_speed_mps):
        """V'_k = V_r (1 - v_k / V_g)."""
        vr = float(platform_speed_mps)
        return vr * (1.0 - self.v_grid() / self.ground_speed(vr))

    def c_params(self, wavelength_m, platform_speed_mps, prf_hz, r0_m, dr_m, cal_phase):
        L, W = self.validate()
        sp = self.speeds(platform_speed_mps)
        if not np.all(sp > 0):
            raise ValueError("the v_along range reaches V' <= 0")
        p = _ffi.RefocusParams()
        p.chip_az, p.chip_rg, p.source, p.n_hyp = L, W, SOURCES[self.source], int(self.n_hyp)
        p.wavelength_m, p.platform_speed_mps, p.prf_hz = float(wavelength_m), float(platform_speed_mps), float(prf_hz)
        p.r0_m, p.dr_m, p.cal_phase = float(r0_m), float(dr_m), float(cal_phase)
        for k, v in enumerate(sp):
            p.speed_mps[k] = float(v)
        return p

    def record_bytes(self, max_detections):
        return int(max_detections) * RECORD_DTYPE.itemsize


class RefocusResult:
    """Per-detection results aligned one-to-one with the detections (`records`, RESULT_DTYPE; result["v_along_mps"] reads a
    field), the hypothesis grid `v_grid` (along-track m/s), and `curves` [n x n_hyp] S_k / `chips` [n x L x W] Y_{k*} when they
    were requested (None otherwise)."""

    def __init__(self, records, v_grid, curves=None, chips=None):
        self.records, self.v_grid, self.curves, self.chips = records, v_grid, curves, chips

    def __len__(self):
        return len(self.records)

    def __getitem__(self, key):
        return self.records[key]

    def __repr__(self):
        return f"RefocusResult(n={len(self)}, hypotheses={len(self.v_grid)})"


def range_geometry(range_axis):
    """(r0, dr) of an affine range axis; ValueError otherwise."""
    ra = np.asarray(range_axis, dtype=np.float64)
    if ra.ndim != 1 or len(ra) < 1:
        raise ValueError("range_axis must be a non-empty 1-D array")
    r0 = float(ra[0])
    dr = float(ra[1] - ra[0]) if len(ra) > 1 else 0.0
    dev = np.abs(ra - (r0 + np.arange(len(ra)) * dr))
    if len(ra) > 2 and not np.all(dev <= 1e-6 * max(abs(dr), 1e-9) + 1e-9 * abs(r0)):
        raise ValueError(f"range_axis is not affine (worst deviation {dev.max():.3g} m from r0 + j dr)")
    return r0, dr


def decode(rec, positions, params, platform_speed_mps, curves=None, chips=None):
    """Raw records [n] (RECORD_DTYPE) of the positions [n x 2] -> RefocusResult."""
    rec = np.ascontiguousarray(rec).view(RECORD_DTYPE).reshape(-1)
    n = len(rec)
    vg = params.v_grid()
    out = np.zeros(n, RESULT_DTYPE)
    pos = np.asarray(positions, dtype=np.int64).reshape(-1, 2)
    out["i"], out["j"] = pos[:, 0], pos[:, 1]
    k = rec["k_best"].astype(np.int64)
    for f in ("k_best", "peak_i", "peak_j", "i0"):
        out[f] = rec[f]
    out["v_along_grid_mps"] = vg[k] if n else []
    step = float(vg[1] - vg[0]) if len(vg) > 1 else 0.0
    sp, sb, sn = (rec[f].astype(np.float64) for f in ("s_prev", "s_best", "s_next"))
    inner = (sp >= 0) & (sn >= 0)
    den = sp - 2.0 * sb + sn
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(inner & (den < 0), 0.5 * (sp - sn) / den, 0.0)     # vertex of the parabola through the three S values
    out["v_along_mps"] = np.clip(out["v_along_grid_mps"] + np.clip(delta, -1.0, 1.0) * step, vg[0], vg[-1])
    out["at_grid_edge"] = (k == 0) | (k == len(vg) - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["refocus_gain_db"] = 10.0 * np.log10(rec["peak_power"].astype(np.float64) / rec["orig_power"].astype(np.float64))
        out["sharpness_gain"] = sb / rec["s_identity"].astype(np.float64)
    out["sharpness"] = sb
    out["sharpness_identity"] = rec["s_identity"]
    return RefocusResult(out, vg, curves, chips)


def enqueue(ctx, d_slc1, d_slc2, n_az, n_rg, cparams, slot_ptr, max_detections, d_records, d_curves=None, d_chips=None):
    """Both refocus launches on the ctx's current lane for the GMTI slot at slot_ptr (header, then the reports); only enqueues."""
    check(ctx.lib.sarx_refocus_dev(ctx.h, d_slc1, d_slc2, int(n_az), int(n_rg), C.byref(cparams), slot_ptr + HEADER_BYTES, slot_ptr,
                                   int(max_detections), d_records, d_curves, d_chips), ctx.h)


class _Outputs:
    """Device buffers of one refocus call: records, and curves / chips when requested."""

    def __init__(self, ctx, params, max_detections):
        L, W = params.validate()
        m = max(int(max_detections), 1)
        self.rec = ctx.alloc(params.record_bytes(m))
        self.curves = ctx.alloc(m * int(params.n_hyp) * 4) if params.want_curves else None
        self.chips = ctx.alloc(m * L * W * 8) if params.want_chips else None
        self.L, self.W, self.n_hyp = L, W, int(params.n_hyp)

    def ptrs(self):
        return self.rec.ptr, (self.curves.ptr if self.curves else None), (self.chips.ptr if self.chips else None)

    def fetch(self, ctx, n):
        rec = _slot.download(ctx, self.rec.ptr, n * RECORD_DTYPE.itemsize).view(RECORD_DTYPE)
        curves = _slot.download(ctx, self.curves.ptr, n * self.n_hyp * 4).view(np.float32).reshape(n, self.n_hyp) if self.curves else None
        chips = _slot.download(ctx, self.chips.ptr, n * self.L * self.W * 8).view(np.complex64).reshape(n, self.L, self.W) if self.chips else None
        return rec, curves, chips

    def release(self):
        for b in (self.rec, self.curves, self.chips):
            if b is not None:
                b.release()


def refocus_slot(ctx, d_slc1, d_slc2, n_az, n_rg, params, range_axis, slot_ptr, max_detections, *, wavelength_m, platform_speed_mps,
                 prf_hz, cal_phase=0.0):
    """Refocus the reports of a device GMTI slot (header + reports) and download the result: the path of
    focus_ati_dpca(detect=..., refocus=...).  Raises GmtiOverflowError when the slot overflowed (nothing was written)."""
    r0, dr = range_geometry(range_axis)
    params.validate(n_az)
    cp = params.c_params(wavelength_m, platform_speed_mps, prf_hz, r0, dr, cal_phase)
    outs = _Outputs(ctx, params, max_detections)
    try:
        enqueue(ctx, d_slc1, d_slc2, n_az, n_rg, cp, slot_ptr, max_detections, *outs.ptrs())
        count = _slot.raise_if_overflowed(*_slot.header(_slot.fetch_header(ctx, slot_ptr)), max_detections, strict=True)
        rep = _slot.download(ctx, slot_ptr + HEADER_BYTES, count * REPORT_DTYPE.itemsize).view(REPORT_DTYPE)
        rec, curves, chips = outs.fetch(ctx, count)
    finally:
        outs.release()
    return decode(rec, np.stack([rep["i"], rep["j"]], axis=1), params, platform_speed_mps, curves, chips)


def positions_slot(positions, n_az, n_rg):
    """A GMTI slot (header + reports carrying only i and j) for an (i, j) array, as bytes."""
    pos = np.asarray(positions)
    if pos.size == 0:
        pos = np.zeros((0, 2), np.int64)
    if pos.ndim != 2 or pos.shape[1] != 2 or not np.issubdtype(pos.dtype, np.integer):
        raise ValueError("positions must be an (n, 2) integer array of (i, j)")
    if len(pos) and ((pos[:, 0] < 0).any() or (pos[:, 0] >= n_az).any() or (pos[:, 1] < 0).any() or (pos[:, 1] >= n_rg).any()):
        raise ValueError("a position lies outside the image")
    rep = np.zeros(len(pos), REPORT_DTYPE)
    rep["i"], rep["j"] = pos[:, 0], pos[:, 1]
    return _slot.encode(rep, max(len(pos), 1)), pos


def gmti_refocus(report_or_positions, slc1, slc2, range_axis, cross_range, *, wavelength_m, platform_speed_mps, prf_hz,
                 params=None, cal_phase=0.0, ctx=None):
    """Estimate the along-track speed of GMTI movers and refocus their images.

    report_or_positions : a GmtiReport (sarx.gmti_detect, focus_ati_dpca(detect=...)), or an (n, 2) int array of (i, j) image
                          positions (i = azimuth row, j = range column)
    slc1, slc2          : [N_rg x N_az] complex host arrays (sar_focus_csa's views) or device images, as gmti_detect takes them;
                          slc2 may be None with params.source = "slc1"
    range_axis, cross_range : the focuser's axes (N_rg, N_az); the range axis must be affine (r0 + j dr)
    platform_speed_mps  : V_r of the focuser's azimuth filter;  params.footprint_speed_mps maps V' to along-track speed
                          (None = V_r, the airborne assumption)
    Returns a RefocusResult aligned with the detections (or positions)."""
    from .engine import default_context
    params = params if params is not None else RefocusParams()
    n_rg, n_az = len(range_axis), len(cross_range)
    params.validate(n_az)
    r0, dr = range_geometry(range_axis)
    cp = params.c_params(wavelength_m, platform_speed_mps, prf_hz, r0, dr, cal_phase)
    if params.source == "dpca" and slc2 is None:
        raise ValueError('source="dpca" needs slc2')
    if isinstance(report_or_positions, GmtiReport):
        d = report_or_positions.detections
        positions = np.stack([d["i"], d["j"]], axis=1).astype(np.int64)
    else:
        positions = report_or_positions
    raw, pos = positions_slot(positions, n_az, n_rg)
    ctx = ctx or getattr(slc1, "ctx", None) or default_context()
    temps = []
    outs = None
    try:
        p1 = _plane_ptr(ctx, slc1, n_az, n_rg, np.complex64, temps)
        p2 = _plane_ptr(ctx, slc2, n_az, n_rg, np.complex64, temps) if slc2 is not None else None
        slot = ctx.to_device(raw)
        temps.append(slot)
        n = len(pos)
        outs = _Outputs(ctx, params, max(n, 1))
        enqueue(ctx, p1, p2, n_az, n_rg, cp, slot.ptr, max(n, 1), *outs.ptrs())
        rec, curves, chips = outs.fetch(ctx, n)
    finally:
        if outs is not None:
            outs.release()
        for b in temps:
            b.release()
    return decode(rec, pos, params, platform_speed_mps, curves, chips)
