"""Focus-velocity search on the two-receiver back-projection, per GMTI report (include/sarx_tdbp_pair_search.h).

``tdbp_pair`` -> ``gmti_detect`` finds movers on the pair's ground grid and gives each a radial speed from the ATI phase.
``tdbp_pair_search`` takes those reports back to the pulses: around every report a small chip of the grid is imaged for both
channels under each of ``n_hyp`` focus velocities in one enqueue, and the sharpness of the chip's DPCA difference I0 - I1 - from
which the stationary clutter has cancelled, unlike the single channel that ``tdbp_search`` sees - names the best hypothesis per
report: the along-track component that ATI cannot see.  The ATI interferogram is taken again at the refocused peak.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi, _tdbp_host as _host, slot as _slot
from ._ffi import check
from .engine import default_context
from .tdbp import batch_constants, cached_plan
from .tdbp_pair import pair_params
from .tdbp_search import RECORD_DTYPE, TdbpSearchResult

BEST_DTYPE = np.dtype([("k_best", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("peak_ix", "<i4"), ("peak_iy", "<i4"), ("reserved", "<i4"),
                       ("s4_prev", "<f8"), ("s4_best", "<f8"), ("s4_next", "<f8"), ("interf_re", "<f8"), ("interf_im", "<f8"),
                       ("p0", "<f8"), ("p1", "<f8")])
assert BEST_DTYPE.itemsize == C.sizeof(_ffi.TdbpPairSearchBest) == 80 and C.sizeof(_ffi.TdbpPairSearchParams) == 16
SOURCES = {"dpca": _ffi.TDBP_PAIR_SEARCH_DPCA, "ch0": _ffi.TDBP_PAIR_SEARCH_CH0}


def search_params(chip, n_hyp, source):
    """The sarx_tdbp_pair_search_params block of chip = (chip_x, chip_y)."""
    if source not in SOURCES:
        raise ValueError(f"source must be one of {tuple(SOURCES)}")
    cx, cy = (int(v) for v in chip)
    return _ffi.TdbpPairSearchParams(cx, cy, int(n_hyp), SOURCES[source])


class TdbpPairSearchResult:
    """Per report r and hypothesis h: ``s2``, ``s4``, ``peak`` [n_reports x n_hyp] (``records`` holds them with the peak's place,
    RECORD_DTYPE of tdbp_search); per report: ``k_best``, the chip's corner ``x0``, ``y0``, the peak of the best hypothesis
    ``peak_ix``, ``peak_iy`` (grid coordinates), ``interf`` = sum I0 conj(I1) over 3 x 3 pixels around it, ``best`` the whole
    record (BEST_DTYPE).  ``chips`` complex128 [n_reports x n_hyp x 2 x chip_y x chip_x] or None.  A report outside the grid has
    k_best = -1 and NaN figures.  ``vel_hyps`` [n_hyp x 3], ``route`` "tile" / "exact", ``lag_s`` as TdbpPairResult has it."""

    def __init__(self, vel_hyps, records, best, chips, route, lag_s, wavelength):
        self.vel_hyps, self.records, self.best, self.chips, self.route = vel_hyps, records, best, chips, route
        self.lag_s, self.wavelength = float(lag_s), float(wavelength)
        self.s2, self.s4, self.peak = records["s2"].copy(), records["s4"].copy(), records["peak"].copy()
        self.k_best, self.x0, self.y0 = best["k_best"].copy(), best["x0"].copy(), best["y0"].copy()
        self.peak_ix, self.peak_iy = best["peak_ix"].copy(), best["peak_iy"].copy()
        self.interf = best["interf_re"] + 1j * best["interf_im"]

    def __len__(self):
        return len(self.best)

    def estimate(self, metric="s4"):
        """Per report the TdbpEstimate of ``TdbpSearchResult.estimate`` on its row of records (None for a report outside the grid)."""
        return [None if self.k_best[r] < 0 else TdbpSearchResult(self.vel_hyps, self.records[r], None, self.route).estimate(metric)
                for r in range(len(self))]

    def v_los(self):
        """Radial speed per report from the interferogram at the refocused peak: -lambda angle(interf) / (4 pi lag)."""
        return -self.wavelength * np.angle(self.interf) / (4.0 * np.pi * self.lag_s)


def tdbp_pair_search(raw1, raw2, pos_tx, vel_tx, rx_offsets, t_start, num_samples, t_pulses, scene_size, nx, ny, reports, vel_hyps, *,
                     chip=(32, 32), source="dpca", chirp_centre=None, pulse_shift=True, chips=False, detect=None, max_detections=None,
                     consts=None, ctx=None):
    """For every report and every focus velocity of ``vel_hyps`` [n_hyp x 3] both channels imaged on a chip of ``tdbp_pair``'s grid
    around the report, in one enqueue on ``tdbp_gpu``'s cached plan.

    raw1 .. ny   : as ``tdbp_pair`` takes them; raw as NumPy arrays or device-resident
    reports      : a GmtiReport (gmti_detect on the pair: row i = iy, column j = ix), a REPORT_DTYPE array, a slot's bytes, or a
                   device slot (anything with .ptr; then ``detect`` or ``max_detections`` gives its capacity)
    chip         : (chip_x, chip_y) pixels, 4 .. 64 each and at most the grid
    source       : "dpca" (the difference I0 - I1) or "ch0" (channel 0 alone)
    chips        : also return both channels of every chip
    Raises GmtiOverflowError when the slot overflowed (nothing was written).  Returns a TdbpPairSearchResult."""
    k = consts or batch_constants()
    ctx = ctx or default_context()
    n_p, n_s, nx, ny = len(t_pulses), int(num_samples), int(nx), int(ny)
    hyp = _host.hypotheses(vel_hyps)
    n_hyp = hyp.shape[0]
    pos, vel, tp, _ = _host.geometry(n_p, pos_tx, vel_tx, t_pulses)
    prm = pair_params(n_p, rx_offsets, _host.chirp_centre(k, chirp_centre), pulse_shift)
    sp = search_params(chip, n_hyp, source)
    lib = ctx.lib
    check(lib.sarx_tdbp_pair_check(n_p, C.byref(prm)))
    check(lib.sarx_tdbp_pair_search_check(C.byref(sp), nx, ny))
    md, stack, on_device = _slot.stage(reports, detect, max_detections, single=True)
    plan = cached_plan(ctx, k, n_p, n_s, nx, ny)
    with _host.temporaries() as held:
        p1, p2 = _host.raw_on_device(ctx, (raw1, raw2), n_p, n_s, held)
        slot_ptr = _host.slot_on_device(ctx, stack, on_device, held)
        n_chip = sp.chip_x * sp.chip_y
        d_rec = _host.hold(held, ctx.alloc(md * n_hyp * RECORD_DTYPE.itemsize))
        d_best = _host.hold(held, ctx.alloc(md * BEST_DTYPE.itemsize))
        d_chips = _host.hold(held, ctx.alloc(md * n_hyp * 2 * n_chip * 16)) if chips else None
        check(lib.sarx_tdbp_pair_search_dev(plan.h, p1, p2, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t_start),
                                            float(scene_size), C.byref(prm), hyp.ctypes.data, slot_ptr + _slot.HEADER_BYTES, slot_ptr, md,
                                            C.byref(sp), d_rec.ptr, d_best.ptr, d_chips.ptr if chips else None), ctx.h)
        count = _slot.raise_if_overflowed(*_slot.header(_slot.fetch_header(ctx, slot_ptr)), md, strict=True)
        best = _slot.download(ctx, d_best.ptr, count * BEST_DTYPE.itemsize).view(BEST_DTYPE).copy()
        rec = _slot.download(ctx, d_rec.ptr, count * n_hyp * RECORD_DTYPE.itemsize).view(RECORD_DTYPE).reshape(count, n_hyp).copy()
        stack_c = None
        if chips:
            stack_c = _slot.download(ctx, d_chips.ptr, count * n_hyp * 2 * n_chip * 16).view(np.complex128).reshape(
                count, n_hyp, 2, sp.chip_y, sp.chip_x).copy()
    out = best["k_best"] < 0                                        # outside the grid: the library wrote k_best alone
    for a, names in ((best, BEST_DTYPE.names[1:]), (rec, RECORD_DTYPE.names)):
        for f in names:
            a[f][out] = -1 if a.dtype[f].kind == "i" else np.nan
    if stack_c is not None:
        stack_c[out] = np.nan
    return TdbpPairSearchResult(hyp.copy(), rec, best, stack_c, _host.route(lib.sarx_tdbp_pair_search_route, plan),
                                _host.lags(rx_offsets, vel)[0], k["C"] / k["FC"])
