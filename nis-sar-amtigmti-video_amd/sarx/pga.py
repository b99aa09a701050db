"""Phase-gradient autofocus on the device (include/sarx_pga.h, csrc/pga.hip).

``pga`` estimates an arbitrary azimuth phase error - one phase per azimuth-frequency bin, in fftshift order - from an image's own
bright points and removes it; ``apply_azimuth_phase`` is the apply step alone, for injecting a known error or for taking a phase
estimated on one frame to another.  A frame is [L x n_rg] with the azimuth axis first (``axis=0``), L in 64 .. 1024 a power of two;
``axis=1`` takes [n_rg x L] through the corner turn on the way in and out.  The semantics are the header's; the host sizes the
buffers and decodes the records.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _ffi, _tdbp_host as _host
from ._ffi import check

RECORD_DTYPE = np.dtype([("s2", "<f8"), ("s4", "<f8"), ("rms_phase", "<f8"), ("n_cols_used", "<i4"), ("n_bins_supported", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(_ffi.PgaRecord) == 32 and C.sizeof(_ffi.PgaParams) == 56


def default_half_widths(n_az, n_iter):
    """L / 4 halved per iteration, with a floor of 3."""
    return [max(3, (int(n_az) // 4) >> it) for it in range(int(n_iter))]


@dataclass
class PgaParams:
    """n_iter: 1 .. 8 estimate-and-apply rounds; half_widths: the window half-width per round (None = ``default_half_widths``);
    min_contrast: a column is used when its peak power is at least this many times its mean power; power_floor: a frequency bin is
    supported when its summed power exceeds this fraction of the largest bin's (in [0, 1))."""
    n_iter: int = 4
    half_widths: Optional[Sequence[int]] = None
    min_contrast: float = 0.0
    power_floor: float = 0.05

    def c_params(self, n_az):
        """The sarx_pga_params block for frames of n_az rows.  Raises ValueError."""
        n_iter = int(self.n_iter)
        if not 1 <= n_iter <= _ffi.PGA_MAX_ITER:
            raise ValueError(f"n_iter {n_iter} must be 1 .. {_ffi.PGA_MAX_ITER}")
        if int(n_az) not in _ffi.PGA_SIZES:
            raise ValueError(f"azimuth length {n_az} must be one of {_ffi.PGA_SIZES}")
        hw = default_half_widths(n_az, n_iter) if self.half_widths is None else [int(h) for h in self.half_widths]
        if len(hw) != n_iter:
            raise ValueError(f"{len(hw)} half-widths for {n_iter} iterations")
        if any(h < 1 or 2 * h + 1 > int(n_az) for h in hw):
            raise ValueError(f"half-widths {hw}: each must be >= 1 with 2 h + 1 <= {n_az}")
        mc, pf = float(self.min_contrast), float(self.power_floor)
        if not (math.isfinite(mc) and mc >= 0.0):
            raise ValueError("min_contrast must be finite and >= 0")
        if not 0.0 <= pf < 1.0:
            raise ValueError("power_floor must be in [0, 1)")
        return _ffi.PgaParams(n_iter, (C.c_int32 * _ffi.PGA_MAX_ITER)(*hw), 0, mc, pf)


def workspace_bytes(cp, n_az, n_rg, ld, n_frames, frame_stride):
    n = C.c_size_t()
    check(_ffi.load().sarx_pga_workspace_bytes(C.byref(cp), int(n_az), int(n_rg), int(ld), int(n_frames), int(frame_stride), C.byref(n)))
    return n.value


def enqueue(ctx, d_in, d_out, n_az, n_rg, ld, n_frames, frame_stride, cp, phase_ptr, records_ptr, workspace_ptr):
    """All launches of one ``sarx_pga_dev`` on the ctx's current lane (device pointers; ld and frame_stride in elements); only enqueues."""
    check(ctx.lib.sarx_pga_dev(ctx.h, d_in, d_out, int(n_az), int(n_rg), int(ld), int(n_frames), int(frame_stride), C.byref(cp), phase_ptr,
                               records_ptr, workspace_ptr), ctx.h)


def enqueue_apply(ctx, d_in, d_out, n_az, n_rg, ld, n_frames, frame_stride, phase_ptr, phase_stride, sign):
    """The apply launch alone (``sarx_pga_apply_dev``); only enqueues."""
    check(ctx.lib.sarx_pga_apply_dev(ctx.h, d_in, d_out, int(n_az), int(n_rg), int(ld), int(n_frames), int(frame_stride), phase_ptr,
                                     int(phase_stride), int(sign)), ctx.h)


class PgaResult:
    """``image``: the corrected frame or stack, of the input's kind and shape (a DeviceBuffer for a device input; release() it);
    ``phase``: phi_tot [L], or [n_frames x L] for a stack, radians over the azimuth-frequency bins in fftshift order;
    ``records``: RECORD_DTYPE [n_iter + 1] (or [n_frames x (n_iter + 1)]): record it describes g_it, the last one the output;
    ``sharpness``: s4 / s2^2 of each record."""

    def __init__(self, image, phase, records):
        self.image, self.phase, self.records = image, phase, records
        with np.errstate(invalid="ignore", divide="ignore"):
            self.sharpness = np.where(records["s2"] > 0, records["s4"] / np.maximum(records["s2"], 1e-300) ** 2, 0.0)

    def release(self):
        if hasattr(self.image, "release"):
            self.image.release()

    def __repr__(self):
        r = np.atleast_2d(self.records)
        return f"PgaResult({r.shape[0]} frame(s), residual rms {float(r[:, -1]['rms_phase'].max()):.3g} rad)"


def _stage(ctx, image, axis, shape, held):
    """The input as a contiguous device stack [n_frames x L x n_rg]: (pointer, n_frames, L, n_rg, stacked, on_device)."""
    if axis not in (0, 1):
        raise ValueError("axis must be 0 (frames are [L x n_rg]) or 1 ([n_rg x L])")
    on_device = hasattr(image, "ptr")
    if on_device:
        shp = tuple(int(x) for x in (shape if shape is not None else getattr(image, "shape", ())))
        if getattr(image, "transposed", False):
            raise ValueError("a transposed device view is not contiguous: pass its base with the other axis")
        if len(shp) not in (2, 3):
            raise ValueError("a device image needs a 2-D or 3-D shape (a DeviceArray, or shape=...)")
        if getattr(image, "nbytes", int(np.prod(shp)) * 8) < int(np.prod(shp)) * 8:
            raise ValueError("device buffer smaller than the image")
        ptr = image.ptr
    else:
        arr = np.asarray(image)
        if arr.ndim not in (2, 3) or not np.iscomplexobj(arr):
            raise ValueError("an image is a complex array, 2-D (one frame) or 3-D (a stack)")
        shp = arr.shape
    stacked = len(shp) == 3
    nf = shp[0] if stacked else 1
    rows, cols = shp[-2], shp[-1]
    n_az, n_rg = (rows, cols) if axis == 0 else (cols, rows)
    if n_az not in _ffi.PGA_SIZES:
        raise ValueError(f"azimuth length {n_az} must be one of {_ffi.PGA_SIZES}")
    if nf < 1 or n_rg < 1:
        raise ValueError("empty image")
    if axis == 1 and (rows % 32 or cols % 32):
        raise ValueError("axis=1 goes through the corner turn: both sides must be multiples of 32")
    if not on_device:
        ptr = _host.hold(held, ctx.to_device(np.ascontiguousarray(arr, dtype=np.complex64))).ptr
    if axis == 1:
        turned = _host.hold(held, ctx.alloc(nf * n_az * n_rg * 8))
        _turn(ctx, ptr, turned.ptr, nf, rows, cols)
        ptr = turned.ptr
    return ptr, nf, n_az, n_rg, stacked, on_device


def _turn(ctx, src, dst, n_frames, rows, cols):
    for f in range(n_frames):
        check(ctx.lib.sarx_corner_turn_dev(ctx.h, src + f * rows * cols * 8, dst + f * rows * cols * 8, int(rows), int(cols)), ctx.h)


def _finish(ctx, out, nf, n_az, n_rg, axis, stacked, on_device, held):
    """The output stack [n_frames x L x n_rg] in the input's kind and shape; ``out`` is kept when it is what is returned."""
    if axis == 1:
        back = ctx.alloc(nf * n_az * n_rg * 8)
        try:
            _turn(ctx, out.ptr, back.ptr, nf, n_az, n_rg)
        except Exception:
            back.release()
            raise
        _host.hold(held, out)
        out = back
    if on_device:
        return out
    _host.hold(held, out)
    shp = (n_az, n_rg) if axis == 0 else (n_rg, n_az)
    img = np.array(out.download(np.complex64, (nf,) + shp))
    return img if stacked else img[0]


def pga(image, params=None, *, axis=0, ctx=None, shape=None):
    """Phase-gradient autofocus of one frame (2-D) or of every frame of a stack (3-D).

    image  : a complex NumPy array, or a device image (a DeviceArray, or anything with .ptr and shape=(.., rows, cols)), complex64
             row-major; ``axis`` names the azimuth axis of a frame: 0 = [L x n_rg], 1 = [n_rg x L].  axis=1 goes through
             sarx_corner_turn_dev on the way in and out, so both sides of a frame must then be multiples of 32 (ValueError otherwise)
    params : PgaParams (None = the defaults)
    The records' s4 is a sum of fp32 products |g|^4: scale a frame whose magnitudes exceed about 1e9 before the call.
    Returns a PgaResult."""
    from .engine import default_context
    params = params or PgaParams()
    ctx = ctx or getattr(image, "ctx", None) or default_context()
    with _host.temporaries() as held:
        ptr, nf, n_az, n_rg, stacked, on_device = _stage(ctx, image, axis, shape, held)
        cp = params.c_params(n_az)
        stride = n_az * n_rg
        check(ctx.lib.sarx_pga_check(C.byref(cp), n_az, n_rg, n_rg, nf, stride))
        n_rec = cp.n_iter + 1
        phase = _host.hold(held, ctx.alloc(nf * n_az * 8))
        rec = _host.hold(held, ctx.alloc(nf * n_rec * RECORD_DTYPE.itemsize))
        work = _host.hold(held, ctx.alloc(max(workspace_bytes(cp, n_az, n_rg, n_rg, nf, stride), 8)))
        out = ctx.alloc(nf * stride * 8)
        try:
            enqueue(ctx, ptr, out.ptr, n_az, n_rg, n_rg, nf, stride, cp, phase.ptr, rec.ptr, work.ptr)
        except Exception:
            out.release()
            raise
        img = _finish(ctx, out, nf, n_az, n_rg, axis, stacked, on_device, held)
        ph = np.array(phase.download(np.float64, (nf, n_az)))
        records = np.array(rec.download(np.uint8, (nf * n_rec * RECORD_DTYPE.itemsize,))).view(RECORD_DTYPE).reshape(nf, n_rec)
        return PgaResult(img, ph if stacked else ph[0], records if stacked else records[0])


def apply_azimuth_phase(image, phase, sign=-1, axis=0, *, ctx=None, shape=None):
    """ifft(fft(image) exp(j sign phase)) along the azimuth axis: sign = -1 removes the phase, +1 puts it in.

    phase : [L] radians over the azimuth-frequency bins in fftshift order (one phase for every frame), or [n_frames x L]
    axis  : as in ``pga``; axis=1 needs both sides of a frame to be multiples of 32
    Returns the image in the input's kind and shape (a DeviceBuffer for a device input)."""
    from .engine import default_context
    if sign not in (-1, 1):
        raise ValueError("sign must be -1 (correct) or +1 (inject)")
    ctx = ctx or getattr(image, "ctx", None) or default_context()
    ph = np.ascontiguousarray(phase, dtype=np.float64)
    with _host.temporaries() as held:
        ptr, nf, n_az, n_rg, stacked, on_device = _stage(ctx, image, axis, shape, held)
        if ph.shape not in ((n_az,), (nf, n_az)):
            raise ValueError(f"phase must be [{n_az}] or [{nf} x {n_az}]")
        if not np.all(np.isfinite(ph)):
            raise ValueError("phase must be finite")
        d_ph = _host.hold(held, ctx.to_device(ph))
        out = ctx.alloc(nf * n_az * n_rg * 8)
        try:
            enqueue_apply(ctx, ptr, out.ptr, n_az, n_rg, n_rg, nf, n_az * n_rg, d_ph.ptr, n_az if ph.ndim == 2 else 0, sign)
        except Exception:
            out.release()
            raise
        return _finish(ctx, out, nf, n_az, n_rg, axis, stacked, on_device, held)
