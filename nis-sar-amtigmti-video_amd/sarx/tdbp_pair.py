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

from . import _ffi
from ._ffi import check
from .engine import DeviceArray, DeviceBuffer, default_context
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


def _raw_ptr(x, n_p, n_s, keep):
    if isinstance(x, (DeviceBuffer, DeviceArray)):
        if isinstance(x, DeviceArray) and (x.shape != (n_p, n_s) or x.transposed):
            raise ValueError(f"device raw must be [{n_p} x {n_s}] row-major")
        if x.nbytes < n_p * n_s * 8:
            raise ValueError("device raw smaller than [n_pulses x num_samples] complex64")
        return x.ptr, True
    a = np.ascontiguousarray(x, dtype=np.complex64)
    if a.shape != (n_p, n_s):
        raise ValueError(f"raw must be [{n_p} x {n_s}]")
    keep.append(a)
    return a.ctypes.data, False


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
    n_p, n_s, nx, ny = len(t_pulses), int(num_samples), int(nx), int(ny)
    dtype = np.dtype(dtype or (np.complex64 if device_output else np.complex128))
    if dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)) or (device_output and dtype != np.dtype(np.complex64)):
        raise ValueError("dtype must be complex128 or complex64 (complex64 with device_output)")
    pos = np.ascontiguousarray(pos_tx, dtype=np.float64)
    vel = np.ascontiguousarray(vel_tx, dtype=np.float64)
    tp = np.ascontiguousarray(t_pulses, dtype=np.float64)
    vf = np.ascontiguousarray(vel_focus, dtype=np.float64)
    if pos.shape != (n_p, 3) or vel.shape != (n_p, 3) or tp.shape != (n_p,) or vf.shape != (3,):
        raise ValueError("pos_tx/vel_tx must be [n_pulses x 3], t_pulses [n_pulses], vel_focus [3]")
    prm = pair_params(n_p, rx_offsets, k["T_P"] / 2 if chirp_centre is None else chirp_centre, pulse_shift)
    check(ctx.lib.sarx_tdbp_pair_check(n_p, C.byref(prm)))
    plan = cached_plan(ctx, k, n_p, n_s, nx, ny)
    keep = []
    p1, dev1 = _raw_ptr(raw1, n_p, n_s, keep)
    p2, dev2 = _raw_ptr(raw2, n_p, n_s, keep)
    if dev1 != dev2:
        raise ValueError("raw1 and raw2 must both be host arrays or both device-resident")
    if device_output and not dev1:
        raise ValueError("device_output needs device-resident raw")
    wide = dtype == np.dtype(np.complex128)
    args = (pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t_start), vf.ctypes.data, float(scene_size), C.byref(prm))
    lib = ctx.lib
    check(lib.sarx_tdbp_search_set_chunks(plan.h, 0 if chunks is None else int(chunks)), ctx.h)      # the plan's chunk count serves both
    if dev1:
        buf = ctx.alloc(2 * ny * nx * dtype.itemsize)
        try:
            check(lib.sarx_tdbp_pair_dev(plan.h, p1, p2, *args, buf.ptr if wide else None, None if wide else buf.ptr), ctx.h)
            if device_output:
                imgs = (DeviceArray(buf, (ny, nx)), DeviceArray(buf, (ny, nx), offset=ny * nx * 8, owner=False))
            else:
                imgs = buf.download(dtype, (2, ny, nx))
        finally:
            if not device_output:
                buf.release()
    else:
        imgs = np.empty((2, ny, nx), dtype=dtype)
        check(lib.sarx_tdbp_pair_host(plan.h, p1, p2, *args, imgs.ctypes.data if wide else None, None if wide else imgs.ctypes.data), ctx.h)
    tile = C.c_int()
    check(lib.sarx_tdbp_pair_route(plan.h, C.byref(tile)), ctx.h)
    off = np.asarray(rx_offsets, dtype=np.float64)
    speed = float(np.mean(np.linalg.norm(vel, axis=1)))
    # the phase centres (midway between transmitter and receiver) lie (off2 - off1) / 2 apart along track: the second one passes
    # a point this much later (with offsets -+ V / PRF and the DPCA pulse shift: exactly one pulse interval)
    lag = (off[1] - off[0]) / (2.0 * speed)
    return TdbpPairResult(imgs[0], imgs[1], lag, k["C"] / k["FC"], "tile" if tile.value else "exact", ctx)
