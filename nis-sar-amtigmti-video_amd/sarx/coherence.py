"""Sliding-window coherence on the GPU: the complex sample coherence of two complex64 images over a box around every pixel
(include/sarx_coherence.h, csrc/coherence.hip), for masking ATI phase and for coherent change detection between VideoSAR frames.

Semantics (the kernel implements them; the host sizes the buffers and decodes the summary):
  window = (ha, hr): the box |di| <= ha (azimuth), |dj| <= hr (range) around a pixel, clipped to the image, N cells.  Over it, in
  fp64: S12 = sum a conj(b), S11 = sum |a|^2, S22 = sum |b|^2; g = S12 / sqrt(S11 S22), 0 where S11 S22 = 0.  coh = |g| (fp32,
  at most 1), igram = g (complex64).  With a threshold a pixel is tested when S11 >= power_floor N and S22 >= power_floor N, and
  changed when it is tested and coh < threshold; mask: 0 = not tested, 1 = tested and unchanged, 2 = changed.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from ._ffi import check

SUMMARY_BYTES = C.sizeof(_ffi.CoherenceSummary)
SUMMARY_DTYPE = np.dtype([("n_tested", "<u8"), ("n_changed", "<u8"), ("sum_coh", "<f8"), ("n_az", "<u4"), ("n_rg", "<u4"),
                          ("reserved", "<u4", (8,))])
assert SUMMARY_DTYPE.itemsize == SUMMARY_BYTES == 64


@dataclass
class CoherenceParams:
    """window (ha, hr): half-widths along azimuth and range, 0 .. 16 each; threshold: a tested pixel whose coherence is below it is
    changed (None = no change rule: no mask and no counts unless asked for, and then nothing is changed); power_floor: mean power
    per cell both images need over the window for the pixel to be tested."""
    window: Tuple[int, int] = (2, 2)
    threshold: Optional[float] = None
    power_floor: float = 0.0

    def check(self):
        """Returns (ha, hr).  Raises ValueError."""
        try:
            ha, hr = (int(x) for x in self.window)
        except (TypeError, ValueError):
            raise ValueError("window must be (ha, hr)") from None
        if not (0 <= ha <= _ffi.COH_MAX_HALF and 0 <= hr <= _ffi.COH_MAX_HALF):
            raise ValueError(f"window half-widths {ha}, {hr}: each must be 0 .. {_ffi.COH_MAX_HALF}")
        if self.threshold is not None and not (math.isfinite(float(self.threshold)) and float(self.threshold) >= 0.0):
            raise ValueError("threshold must be finite and >= 0 (None = no change rule)")
        if not (math.isfinite(float(self.power_floor)) and float(self.power_floor) >= 0.0):
            raise ValueError("power_floor must be finite and >= 0")
        return ha, hr

    def c_params(self):
        ha, hr = self.check()
        return _ffi.CoherenceParams(ha, hr, 0, 0, 0.0 if self.threshold is None else float(self.threshold), float(self.power_floor))


def workspace_bytes(cp, n_az, n_rg):
    n = C.c_size_t()
    check(_ffi.load().sarx_coherence_workspace_bytes(C.byref(cp), int(n_az), int(n_rg), C.byref(n)))
    return n.value


def enqueue_pair(ctx, d_a, d_b, n_az, n_rg, cp, coh_ptr, igram_ptr=None, mask_ptr=None, summary_ptr=None, workspace_ptr=None):
    """One pair's launches on the ctx's current lane (device pointers, [n_az x n_rg] row-major); only enqueues."""
    check(ctx.lib.sarx_coherence_pair_dev(ctx.h, d_a, d_b, int(n_az), int(n_rg), C.byref(cp), coh_ptr, igram_ptr, mask_ptr, summary_ptr,
                                          workspace_ptr), ctx.h)


def enqueue_stack(ctx, d_frames, n_frames, frame_stride, lag, n_az, n_rg, cp, coh_ptr, coh_stride, igram_ptr=None, igram_stride=0,
                  mask_ptr=None, mask_stride=0, summary_ptr=None, workspace_ptr=None):
    """The launches of the pairs (f, f + lag) of a device stack; strides in bytes; only enqueues."""
    check(ctx.lib.sarx_coherence_stack_dev(ctx.h, d_frames, int(n_frames), int(frame_stride), int(lag), int(n_az), int(n_rg), C.byref(cp),
                                           coh_ptr, int(coh_stride), igram_ptr, int(igram_stride), mask_ptr, int(mask_stride), summary_ptr,
                                           workspace_ptr), ctx.h)


class CoherenceResult:
    """coh (fp32), igram (complex64 or None), mask (uint8 or None) as planes of the input's kind (host arrays, or DeviceBuffers
    [n_az x n_rg] row-major with device_output; release() them); n_tested, n_changed, mean_coh (the mean coherence of the tested
    pixels, nan when there is none) when the change rule ran, else None.  From coherence_stack the planes carry a leading pair axis
    and the three figures are arrays, one entry per pair."""

    def __init__(self, coh=None, igram=None, mask=None, summary=None):
        self.coh, self.igram, self.mask = coh, igram, mask
        self.n_tested = self.n_changed = self.mean_coh = None
        self.summary = summary
        if summary is not None:
            s = np.atleast_1d(summary)
            nt, nc = s["n_tested"].astype(np.int64), s["n_changed"].astype(np.int64)
            with np.errstate(invalid="ignore", divide="ignore"):
                mean = np.where(nt > 0, s["sum_coh"] / np.maximum(nt, 1), np.nan)
            if np.ndim(summary) == 0:
                self.n_tested, self.n_changed, self.mean_coh = int(nt[0]), int(nc[0]), float(mean[0])
            else:
                self.n_tested, self.n_changed, self.mean_coh = nt, nc, mean

    def release(self):
        for b in (self.coh, self.igram, self.mask):
            if hasattr(b, "release"):
                b.release()

    def __repr__(self):
        return f"CoherenceResult(n_tested={self.n_tested}, n_changed={self.n_changed}, mean_coh={self.mean_coh})"


def coherence_dev(ctx, p_a, p_b, n_az, n_rg, params, *, igram=False, mask=False, summary=False):
    """Allocates the planes and enqueues one pair on device pointers.  Returns {"coh", "igram", "mask", "summary", "workspace"}
    DeviceBuffers (None where not asked for; release the workspace once the lane has run); nothing is downloaded."""
    cp = params.c_params()
    n = int(n_az) * int(n_rg)
    out = {"coh": None, "igram": None, "mask": None, "summary": None, "workspace": None}
    try:
        out["coh"] = ctx.alloc(n * 4)
        if igram:
            out["igram"] = ctx.alloc(n * 8)
        if mask:
            out["mask"] = ctx.alloc(n)
        if summary:
            out["summary"] = ctx.alloc(SUMMARY_BYTES)
            out["workspace"] = ctx.alloc(max(workspace_bytes(cp, n_az, n_rg), 8))
        ptr = {k: (v.ptr if v is not None else None) for k, v in out.items()}
        enqueue_pair(ctx, p_a, p_b, n_az, n_rg, cp, ptr["coh"], ptr["igram"], ptr["mask"], ptr["summary"], ptr["workspace"])
    except Exception:
        for b in out.values():
            if b is not None:
                b.release()
        raise
    return out


def coherence(a, b, params=None, *, ctx=None, igram=False, mask=False, device_output=False, shape=None):
    """Coherence of two images over a sliding window.

    a, b          : host [N_rg x N_az] complex arrays (sar_focus_csa's views) or device images ([N_az x N_rg] DeviceArray, or
                    DeviceBuffer with shape=(n_az, n_rg)), both of the same kind
    igram, mask   : also the complex coherence / the change mask (the change rule and the counts run with mask=True or a
                    threshold in params)
    device_output : the planes stay on the GPU as [n_az x n_rg] DeviceBuffers
    Returns a CoherenceResult; host planes come back as [N_rg x N_az] views like the inputs."""
    from .balance import _image
    from .engine import default_context
    params = params or CoherenceParams()
    params.check()
    host = not (hasattr(a, "ptr") and hasattr(b, "ptr"))
    if host:
        a1, a2 = np.asarray(a), np.asarray(b)
        if a1.ndim != 2 or a1.shape != a2.shape:
            raise ValueError("a and b must be 2-D images of the same shape and kind")
        if not (np.iscomplexobj(a1) and np.iscomplexobj(a2)):
            raise ValueError("host images are complex arrays [N_rg x N_az] like sar_focus_csa's result")
    ctx = ctx or getattr(a, "ctx", None) or default_context()
    want_summary = mask or params.threshold is not None
    temps = []
    try:
        p1, n_az, n_rg, kind = _image(ctx, a, temps, shape)
        p2, n_az2, n_rg2, kind2 = _image(ctx, b, temps, shape)
        if (n_az, n_rg, kind) != (n_az2, n_rg2, kind2):
            raise ValueError("a and b must be images of the same shape and kind")
        out = coherence_dev(ctx, p1, p2, n_az, n_rg, params, igram=igram, mask=mask, summary=want_summary)
        try:
            sm = None
            if want_summary:
                sm = out["summary"].download(np.uint8, (SUMMARY_BYTES,)).copy().view(SUMMARY_DTYPE)[0]
            if device_output:
                planes = {k: out[k] for k in ("coh", "igram", "mask")}
                out = {"summary": out["summary"], "workspace": out["workspace"]}
            else:
                types = {"coh": np.float32, "igram": np.complex64, "mask": np.uint8}
                planes = {k: (np.array(out[k].download(t, (n_az, n_rg))).T if out[k] is not None else None) for k, t in types.items()}
            return CoherenceResult(planes["coh"], planes["igram"], planes["mask"], sm)
        finally:
            for v in out.values():
                if v is not None:
                    v.release()
    finally:
        for t in temps:
            t.release()


def coherence_stack(frames, params=None, lag=1, *, ctx=None, igram=False, mask=False, maps=True, device_output=False, shape=None):
    """Coherence of the pairs (f, f + lag) of a stack of frames on one ground grid.

    frames : host [n_frames x n_az x n_rg] complex array (one upload) or a DeviceBuffer holding that stack with
             shape=(n_frames, n_az, n_rg)
    maps   : False = only the summaries come back (the change rule runs; no plane is kept)
    Returns a CoherenceResult whose planes are [n_frames - lag x n_az x n_rg] (one download each; DeviceBuffers with device_output)
    and whose n_tested, n_changed, mean_coh are arrays with one entry per pair (with mask=True, a threshold, or maps=False)."""
    from .engine import default_context
    params = params or CoherenceParams()
    cp = params.c_params()
    lag = int(lag)
    temps = []
    if hasattr(frames, "ptr"):
        if shape is None or len(shape) != 3:
            raise ValueError("a device stack needs shape=(n_frames, n_az, n_rg)")
        nf, n_az, n_rg = (int(x) for x in shape)
        if getattr(frames, "nbytes", nf * n_az * n_rg * 8) < nf * n_az * n_rg * 8:
            raise ValueError("device buffer smaller than the stack")
        ctx = ctx or frames.ctx
        d_frames = frames.ptr
    else:
        arr = np.asarray(frames)
        if arr.ndim != 3 or not np.iscomplexobj(arr):
            raise ValueError("a host stack is a complex array [n_frames x n_az x n_rg]")
        nf, n_az, n_rg = arr.shape
    if nf < 2 or not 1 <= lag < nf:
        raise ValueError(f"{nf} frames with lag {lag}: needs 1 <= lag < n_frames")
    ctx = ctx or default_context()
    if not hasattr(frames, "ptr"):
        buf = ctx.to_device(np.ascontiguousarray(arr, dtype=np.complex64))
        temps.append(buf)
        d_frames = buf.ptr
    n, pairs = n_az * n_rg, nf - lag
    want_summary = mask or params.threshold is not None or not maps
    out = {"coh": None, "igram": None, "mask": None}
    try:
        out["coh"] = ctx.alloc(n * 4 * (pairs if maps else 1))
        if igram and maps:
            out["igram"] = ctx.alloc(n * 8 * pairs)
        if mask and maps:
            out["mask"] = ctx.alloc(n * pairs)
        sm_buf = ws = None
        if want_summary:
            sm_buf = ctx.alloc(SUMMARY_BYTES * pairs)
            ws = ctx.alloc(max(workspace_bytes(cp, n_az, n_rg), 8))
            temps += [sm_buf, ws]
        ptr = {k: (v.ptr if v is not None else None) for k, v in out.items()}
        if maps:
            enqueue_stack(ctx, d_frames, nf, n * 8, lag, n_az, n_rg, cp, ptr["coh"], n * 4, ptr["igram"], n * 8, ptr["mask"], n,
                          sm_buf.ptr if sm_buf else None, ws.ptr if ws else None)
        else:                                   # one plane, overwritten pair after pair on the lane
            for f in range(pairs):
                enqueue_pair(ctx, d_frames + f * n * 8, d_frames + (f + lag) * n * 8, n_az, n_rg, cp, ptr["coh"], None, None,
                             sm_buf.ptr + f * SUMMARY_BYTES, ws.ptr)
        sm = sm_buf.download(np.uint8, (SUMMARY_BYTES * pairs,)).copy().view(SUMMARY_DTYPE) if want_summary else None
        if not maps:
            return CoherenceResult(summary=sm)
        if device_output:
            planes, out = dict(out), {}
        else:
            types = {"coh": np.float32, "igram": np.complex64, "mask": np.uint8}
            planes = {k: (np.array(out[k].download(t, (pairs, n_az, n_rg))) if out[k] is not None else None) for k, t in types.items()}
        return CoherenceResult(planes["coh"], planes["igram"], planes["mask"], sm)
    finally:
        for v in list(out.values()) + temps:
            if v is not None:
                v.release()
