"""Two-receiver back-projection (include/sarx_tdbp_pair.h).

``tdbp_pair`` images both receive channels of the two-receiver echo model (``run_bistatic_physics_gpu``,
sar_ati_dcpa_sim_csa.py:113-178) onto one ground grid in one launch.  The pair is co-registered pixel for pixel, so it goes
straight into ``ati_dpca`` and the GMTI chain, and the ATI phase of a pixel, ``angle(I0 conj(I1)) = -4 pi v_los lag / lambda``
with ``lag = (off1 - off0) / (2 |v_tx|)``, is the radial speed that the focus-velocity search (``tdbp_search``) cannot see.

A note on the sample rate: ``run_bistatic_physics_gpu`` spaces its fast-time grid by ``window / (N - 1)`` (:113), not by
``1 / FS``.  A caller who wants the compressed envelope placed exactly passes ``FS * (N - 1) / N`` as the plan's sample rate
(``consts["FS"]``); with the nominal FS the envelope is off by up to one sample at the end of the window, the carrier phase
is not affected.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi, _tdbp_host as _host
from .engine import DeviceArray, default_context
from .tdbp import batch_constants, cached_plan


class TdbpPairResult:
    """``img1``, ``img2`` [ny x nx]: NumPy arrays, or complex64 DeviceArrays with ``device_output``; ``lag_s`` the time between
    the two phase centres, ``v_ambiguity`` = lambda / (4 lag) the span of unambiguous radial speed, ``route`` "exact" / "tile"."""

    def __init__(self, img1, img2, lag_s, wavelength, route, ctx):
        self.img1, self.img2, self.lag_s, self.wavelength, self.route, self.ctx = img1, img2, float(lag_s), float(wavelength), route, ctx
        self.v_ambiguity = self.wavelength / (4.0 * abs(self.lag_s)) if self.lag_s else float("inf")

    def v_los(self, phase):
        """Radial speed of an ATI phase angle(I0 conj(I1)): -lambda phase / (4 pi lag)."""
        return -self.wavelength * np.asarray(phase, dtype=np.float64) / (4.0 * np.pi * self.lag_s)

    def ati_dpca(self, mask_frac=0.05, cal_phase=0.0, **kw):
        """``sarx.ati_dpca`` on the pair (its complex64 form; a complex128 host pair is rounded here).  A device-resident pair
        goes into the same ATI / DPCA launch where it lies; the planes ati_phase, slc1_mag, dpca_mag, ati_phase_masked and mask,
        max_mag, sum_interf come back as ``sarx.ati_dpca`` returns them."""
        from .focus import ati_dpca
        a, b = self.img1, self.img2
        if not isinstance(a, DeviceArray):
            return ati_dpca(a.astype(np.complex64), b.astype(np.complex64), mask_frac, cal_phase, ctx=self.ctx, **kw)
        if kw:
            raise ValueError("a device-resident pair gives the three planes and the masked phase only")
        ctx, n = self.ctx, a.shape[0] * a.shape[1]
        outs = {k: ctx.alloc(n * 4) for k in ("ati_phase", "slc1_mag", "dpca_mag")}
        d_masked = ctx.alloc(n * 4)
        try:
            max_mag, sum_interf = ctx.ati_dpca(a, b, n, cal_phase, outs)
            thr = np.float32(max_mag) * np.float32(mask_frac)
            ctx.mask_phase(outs["ati_phase"], outs["slc1_mag"], n, thr, d_masked)
            res = {k: v.download(np.float32, a.shape) for k, v in outs.items()}
            res["ati_phase_masked"] = d_masked.download(np.float32, a.shape)
        finally:
            for buf in (d_masked, *outs.values()):
                buf.release()
        res.update(mask=res["slc1_mag"] > thr, max_mag=max_mag, sum_interf=sum_interf)
        return res

    def release(self):
        """Frees a device-resident pair."""
        if isinstance(self.img1, DeviceArray):
            self.img1.release()


def pair_params(n_pulses, rx_offsets, chirp_centre, pulse_shift):
    """The sarx_tdbp_pair_params block: ``pulse_shift`` True is the DPCA shift (channel 0 uses pulses 1 .. N-1, channel 1
    0 .. N-2, sar_ati_dcpa_sim_csa.py:402-403), False none, or ((first0, first1), n_used)."""
    if pulse_shift is True:
        first, n_used = (1, 0), n_pulses - 1
    elif pulse_shift is False:
        first, n_used = (0, 0), n_pulses
    else:
        first, n_used = pulse_shift
    off = np.asarray(rx_offsets, dtype=np.float64)
    if off.shape != (2,):
        raise ValueError("rx_offsets must be two distances along the velocity vector")
    return _ffi.TdbpPairParams((C.c_double * 2)(*off), float(chirp_centre), (C.c_int32 * 2)(int(first[0]), int(first[1])), int(n_used), 0)


def tdbp_pair(raw1, raw2, pos_tx, vel_tx, rx_offsets, t_start, num_samples, t_pulses, scene_size, nx=512, ny=512, *,
              vel_focus=(0.0, 0.0, 0.0), chirp_centre=None, pulse_shift=True, consts=None, ctx=None, device_output=False, dtype=None,
              chunks=None):
    """Both channels of one two-receiver CPI back-projected onto the grid of ``tdbp_gpu`` (whose cached plan is shared).

    raw1, raw2   : [n_pulses x num_samples] complex, both NumPy arrays or both device-resident (the DeviceArray of
                   run_bistatic_physics_gpu(device=True), or a DeviceBuffer)
    rx_offsets   : (off1, off2) metres along the unit velocity: receiver c at pos_tx + off_c * vel_tx / |vel_tx|
    chirp_centre : where the compressed peak sits relative to the delay; None = T_P / 2, the chirp of
                   run_bistatic_physics_gpu (it starts at the delay, :166-168); 0 for run_physics_spotlight's
    pulse_shift  : True = the DPCA pulse shift, False = every pulse for both channels, or ((first1, first2), n_used)
    dtype        : np.complex128 (default for host output) or np.complex64 (the fp64 sums rounded once; the only form
                   of ``device_output=True``, which needs device-resident raw and leaves the pair on the GPU)
    chunks       : pulse chunks (None = chosen by the library)
    Returns a TdbpPairResult; its ``route`` tells whether the tile-expanded kernel ran or the exact one."""
    k = consts or batch_constants()
    ctx = ctx or default_context()
    lib, ny, nx = ctx.lib, int(ny), int(nx)
    stack, lags, route = _host.focus_channels(
        lib.sarx_tdbp_pair_check, lib.sarx_tdbp_pair_dev, lib.sarx_tdbp_pair_host, lib.sarx_tdbp_pair_route,
        lambda n_p, off, vel, tp, centre: pair_params(n_p, off, centre, pulse_shift), lambda ptrs: ptrs, cached_plan,
        ctx, k, (raw1, raw2), pos_tx, vel_tx, rx_offsets, t_start, num_samples, t_pulses, scene_size, nx, ny, vel_focus, chirp_centre,
        device_output, dtype, chunks)
    if device_output:                           # two views of the one buffer; the first owns it
        stack = (DeviceArray(stack, (ny, nx)), DeviceArray(stack, (ny, nx), offset=ny * nx * 8, owner=False))
    return TdbpPairResult(stack[0], stack[1], lags[0], k["C"] / k["FC"], route, ctx)
