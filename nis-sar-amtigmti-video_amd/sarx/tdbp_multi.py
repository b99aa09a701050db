"""N-receiver back-projection and the multi-baseline ATI resolver (include/sarx_tdbp_multi.h).

``tdbp_multi`` images two, three or four receive channels of the bistatic echo model (one ``run_bistatic_physics_gpu`` call per
receiver offset) onto one ground grid in one enqueue: a co-registered stack.  Baseline b is the channel pair (0, b) with
``lag = (off_b - off_0) / (2 |v_tx|)``; its ATI phase gives the radial speed modulo ``2 v_ambiguity = lambda / (2 lag)``.  A short
baseline is unambiguous but insensitive, a long one sensitive but wrapped after a few m/s; ``TdbpMultiResult.resolve`` finds, per
GMTI report, the wrap count of the longest baseline under which the others agree (CRT Solver.html:40-51).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi, _tdbp_host as _host, slot as _slot
from ._ffi import check
from .engine import DeviceArray, default_context
from .tdbp import batch_constants, cached_plan
from .tdbp_pair import TdbpPairResult

RECORD_DTYPE = np.dtype([("v_los", "<f8"), ("v_coarse", "<f8"), ("cost", "<f8"), ("cost_next", "<f8"), ("phase", "<f8", (3,)),
                         ("k", "<i4"), ("status", "<u4")])
assert RECORD_DTYPE.itemsize == C.sizeof(_ffi.TdbpMultiRecord) == 64


def aligned_pulse_ranges(rx_offsets, vel_tx, t_pulses):
    """((first_c), n_used) that let every phase centre sweep the same aperture: channel c's phase centre runs (off_c - off_0) / 2
    ahead of channel 0's, m_c = (off_c - off_0) PRF / (2 V) pulses, so it uses the pulses that much earlier.  Raises when an m_c is
    no integer within 1e-6."""
    off = np.asarray(rx_offsets, dtype=np.float64)
    tp = np.asarray(t_pulses, dtype=np.float64)
    if len(tp) < 2:
        raise ValueError("aligned pulse ranges need at least two pulses")
    prf = (len(tp) - 1) / float(tp[-1] - tp[0])
    m = (off - off[0]) * prf / (2.0 * _host.mean_speed(vel_tx))
    mi = np.rint(m)
    if np.any(np.abs(m - mi) > 1e-6):
        raise ValueError(f"the phase centres lie {m.tolist()} pulses apart, not whole pulses: pass pulse_ranges=((first_c ...), n_used)")
    mi = mi.astype(np.int64)
    n_used = len(tp) - int(mi.max() - mi.min())
    if n_used < 1:
        raise ValueError("the phase centres lie further apart than the CPI is long")
    return tuple(int(mi.max() - x) for x in mi), n_used


def multi_params(n_pulses, rx_offsets, chirp_centre, pulse_ranges):
    """The sarx_tdbp_multi_params block; pulse_ranges ((first_c ...), n_used)."""
    off = np.asarray(rx_offsets, dtype=np.float64)
    if off.ndim != 1 or not 2 <= len(off) <= _ffi.TDBP_MULTI_MAX_RX:
        raise ValueError(f"rx_offsets must be 2 .. {_ffi.TDBP_MULTI_MAX_RX} distances along the velocity vector")
    first, n_used = pulse_ranges
    if len(first) != len(off):
        raise ValueError("pulse_ranges needs one first pulse per channel")
    pad = [0] * (_ffi.TDBP_MULTI_MAX_RX - len(off))
    return _ffi.TdbpMultiParams((C.c_double * 4)(*off, *pad), float(chirp_centre), (C.c_int32 * 4)(*(int(f) for f in first), *pad), int(n_used),
                                len(off))


def resolve_params(lags_s, wavelength, v_max, half, max_detections):
    """The sarx_tdbp_multi_resolve_params block of n_rx = len(lags_s) + 1 channels."""
    lags = [float(x) for x in lags_s]
    if not 1 <= len(lags) <= 3:
        raise ValueError("one to three baselines")
    return _ffi.TdbpMultiResolveParams((C.c_double * 3)(*lags, *([0.0] * (3 - len(lags)))), float(wavelength), float(v_max), len(lags) + 1,
                                       int(half), int(max_detections), 0)


class TdbpMultiResult:
    """``imgs``: the stack, a NumPy array [n_rx x ny x nx] or, with ``device_output``, a list of complex64 DeviceArrays that are
    views of one device buffer [n_rx][ny][nx]; ``lags_s`` and ``v_ambiguity`` per baseline b = channels (0, b + 1); ``route``
    "exact" / "tile"."""

    def __init__(self, imgs, lags_s, wavelength, route, ctx, buf=None):
        self.imgs, self.wavelength, self.route, self.ctx, self._buf = imgs, float(wavelength), route, ctx, buf
        self.lags_s = tuple(float(x) for x in lags_s)
        self.v_ambiguity = tuple(self.wavelength / (4.0 * abs(x)) if x else float("inf") for x in self.lags_s)
        self.n_rx = len(self.lags_s) + 1

    def pair(self, b):
        """Channels (0, b), b = 1 .. n_rx - 1, as a TdbpPairResult on the same memory: gmti_detect, ati_dpca and the rest of the chain
        take it unchanged.  The views of a device-resident stack own nothing: the stack's ``release`` frees them."""
        if not 1 <= b < self.n_rx:
            raise ValueError(f"pair(b): b must be 1 .. {self.n_rx - 1}")
        return TdbpPairResult(self.imgs[0], self.imgs[b], self.lags_s[b - 1], self.wavelength, self.route, self.ctx)

    def resolve(self, reports, v_max, half=1, max_detections=None):
        """One record per report (RECORD_DTYPE: v_los, v_coarse, cost, cost_next, phase[3], k, status) from all baselines of the
        stack, on the device.  reports: a GmtiReport, a REPORT_DTYPE array, a slot's bytes, or a device slot (anything with .ptr,
        with ``max_detections`` = its capacity); i = row, j = column of the images.  v_max: the largest |v_los| a wrap count may
        give.  Raises GmtiOverflowError on an overflowed slot."""
        ctx = self.ctx or default_context()
        md, stack, on_device = _slot.stage(reports, max_detections=max_detections, single=True)
        prm = resolve_params(self.lags_s, self.wavelength, v_max, half, md)
        check(ctx.lib.sarx_tdbp_multi_resolve_check(C.byref(prm)))
        with _host.temporaries() as held:
            if isinstance(self.imgs, np.ndarray):
                ny, nx = self.imgs.shape[1:]
                p_img = _host.hold(held, ctx.to_device(np.ascontiguousarray(self.imgs, dtype=np.complex64))).ptr
            else:
                ny, nx = self.imgs[0].shape
                p_img = self.imgs[0].ptr
            p_slot = _host.slot_on_device(ctx, stack, on_device, held)
            rec = _host.hold(held, ctx.alloc(md * RECORD_DTYPE.itemsize))
            check(ctx.lib.sarx_tdbp_multi_resolve_dev(ctx.h, C.byref(prm), p_img, int(ny), int(nx), p_slot, rec.ptr), ctx.h)
            count = _slot.raise_if_overflowed(*_slot.header(_slot.fetch_header(ctx, p_slot)), md, strict=True)
            return _slot.download(ctx, rec.ptr, count * RECORD_DTYPE.itemsize).view(RECORD_DTYPE).copy()

    def release(self):
        """Frees a device-resident stack."""
        if self._buf is not None:
            self._buf.release()
            self._buf = None


def tdbp_multi(raws, pos_tx, vel_tx, rx_offsets, t_start, num_samples, t_pulses, scene_size, nx=512, ny=512, *, vel_focus=(0.0, 0.0, 0.0),
               chirp_centre=None, pulse_ranges=None, consts=None, ctx=None, device_output=False, dtype=None, chunks=None):
    """Two to four receive channels of one CPI back-projected onto the grid of ``tdbp_gpu`` (whose cached plan is shared).

    raws         : n_rx arrays [n_pulses x num_samples] complex, all NumPy arrays or all device-resident
    rx_offsets   : n_rx distances along the unit velocity: receiver c at pos_tx + off_c * vel_tx / |vel_tx|
    chirp_centre : None = T_P / 2, the chirp of run_bistatic_physics_gpu; 0 for run_physics_spotlight's
    pulse_ranges : ((first_c ...), n_used), or None = the ranges that align the phase centres (aligned_pulse_ranges; it raises
                   when the offsets are not whole pulses apart)
    dtype, device_output, chunks : as for ``tdbp_pair``
    Returns a TdbpMultiResult."""
    k = consts or batch_constants()
    ctx = ctx or default_context()
    lib, ny, nx = ctx.lib, int(ny), int(nx)
    stack, lags, route = _host.focus_channels(
        lib.sarx_tdbp_multi_check, lib.sarx_tdbp_multi_dev, lib.sarx_tdbp_multi_host, lib.sarx_tdbp_multi_route,
        lambda n_p, off, vel, tp, centre: multi_params(n_p, off, centre,
                                                       aligned_pulse_ranges(off, vel, tp) if pulse_ranges is None else pulse_ranges),
        lambda ptrs: ((C.c_void_p * len(ptrs))(*ptrs),), cached_plan,
        ctx, k, raws, pos_tx, vel_tx, rx_offsets, t_start, num_samples, t_pulses, scene_size, nx, ny, vel_focus, chirp_centre,
        device_output, dtype, chunks)
    buf = None
    if device_output:                           # views of the one buffer, which the result owns
        buf, stack = stack, [DeviceArray(stack, (ny, nx), offset=c * ny * nx * 8, owner=False) for c in range(len(raws))]
    return TdbpMultiResult(stack, lags, k["C"] / k["FC"], route, ctx, buf)
