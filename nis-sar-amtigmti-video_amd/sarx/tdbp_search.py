"""Focus-velocity search of the VideoSAR back-projection (include/sarx_tdbp_search.h).

The reference's "mBP" mode focuses with the simulation's own target velocity (sar_batch_sim.py:320: ``vel_focus = v_tgt_vec``);
a real CPI has no such vector.  ``tdbp_search`` images one CPI under many focus velocities in one enqueue - the pulses are
range-compressed once - and returns per velocity s2 = sum |I|^2, s4 = sum |I|^4 and the peak power.  Sharpness tells the
ALONG-TRACK component only (a ground-range mismatch displaces the target, it does not defocus it), and only over a long CPI;
``tdbp_velocity_line`` lays hypotheses on a line, ``TdbpSearchResult.estimate`` refines the best one with a three-point parabola,
``tdbp_autofocus`` does both and focuses at the estimate.
"""
from __future__ import annotations

import numpy as np

from . import _ffi, _tdbp_host as _host
from ._ffi import check
from .engine import DeviceBuffer, default_context
from .tdbp import batch_constants, cached_plan, tdbp_gpu

RECORD_DTYPE = np.dtype([("s2", "<f8"), ("s4", "<f8"), ("peak", "<f8"), ("peak_ix", "<i4"), ("peak_iy", "<i4")])
METRICS = ("s4", "peak", "sharpness")


def tdbp_velocity_line(center, direction, half_span, n):
    """[n x 3] hypotheses ``center + s_k * direction / |direction|``, s_k uniform on [-half_span, half_span]; n odd, so the
    centre itself is one of them."""
    center = np.asarray(center, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64)
    n = int(n)
    if center.shape != (3,) or d.shape != (3,):
        raise ValueError("center and direction must be 3-vectors")
    norm = float(np.linalg.norm(d))
    if not (np.isfinite(norm) and norm > 0):
        raise ValueError("direction must be finite and non-zero")
    if n < 1 or n % 2 == 0:
        raise ValueError("n must be odd and >= 1")
    if not (np.isfinite(half_span) and half_span >= 0):
        raise ValueError("half_span must be finite and >= 0")
    s = (np.arange(n) - n // 2) * (float(half_span) / (n // 2) if n > 1 else 0.0)
    return center[None, :] + s[:, None] * (d / norm)[None, :]


def parabola_vertex(y_prev, y_best, y_next):
    """Vertex of the parabola through (-1, y_prev), (0, y_best), (1, y_next) in grid steps, clipped to [-0.5, 0.5]; 0 when the
    three points lie on a line."""
    den = y_prev - 2.0 * y_best + y_next
    if not np.isfinite(den) or den == 0.0:
        return 0.0
    return float(np.clip(0.5 * (y_prev - y_next) / den, -0.5, 0.5))


class TdbpEstimate:
    """``velocity`` [3], ``offset`` along the line from its centre, ``index`` of the best hypothesis, ``edge`` (the best one is
    an end of the line: the maximum may lie outside), ``metric``."""

    def __init__(self, velocity, offset, index, edge, metric):
        self.velocity, self.offset, self.index, self.edge, self.metric = velocity, float(offset), int(index), bool(edge), metric

    def __repr__(self):
        return f"TdbpEstimate(velocity={self.velocity}, offset={self.offset}, index={self.index}, edge={self.edge}, metric={self.metric!r})"


class TdbpSearchResult:
    """Per hypothesis: ``vel_hyps`` [n x 3], ``s2``, ``s4``, ``peak`` (fp64), ``peak_ix``, ``peak_iy`` (int32); ``images``
    complex128 [n x ny x nx] or None; ``route`` "tile" / "exact": the kernel the search took."""

    def __init__(self, vel_hyps, records, images, route):
        self.vel_hyps = vel_hyps
        self.records = records
        self.s2, self.s4, self.peak = records["s2"].copy(), records["s4"].copy(), records["peak"].copy()
        self.peak_ix, self.peak_iy = records["peak_ix"].copy(), records["peak_iy"].copy()
        self.images = images
        self.route = route

    def metric(self, name="s4"):
        if name == "s4":
            return self.s4
        if name == "peak":
            return self.peak
        if name == "sharpness":
            return self.s4 / (self.s2 * self.s2)
        raise ValueError(f"metric must be one of {METRICS}")

    def estimate(self, metric="s4"):
        """Argmax b of the metric; for an interior b on a uniform line s* = s_b + step * vertex of the parabola through the three
        points around b, clipped to half a step; at an end of the line s_b and edge=True.  Host fp64 on n numbers."""
        y = np.asarray(self.metric(metric), dtype=np.float64)
        if not np.isfinite(y).all():
            raise ValueError("the metric is not finite for every hypothesis")
        v = self.vel_hyps
        n = len(y)
        b = int(np.argmax(y))
        if n == 1:
            return TdbpEstimate(v[0].copy(), 0.0, 0, True, metric)
        step_vec = (v[-1] - v[0]) / (n - 1)
        step = float(np.linalg.norm(step_vec))
        if not np.allclose(v, v[0][None, :] + np.arange(n)[:, None] * step_vec[None, :], rtol=0, atol=1e-9 * max(step, 1e-300) + 1e-12):
            raise ValueError("estimate needs hypotheses on a uniform line (tdbp_velocity_line)")
        s_b = (b - (n - 1) / 2.0) * step
        if b == 0 or b == n - 1:
            return TdbpEstimate(v[b].copy(), s_b, b, True, metric)
        frac = parabola_vertex(y[b - 1], y[b], y[b + 1])
        return TdbpEstimate(v[b] + frac * step_vec, s_b + frac * step, b, False, metric)


def tdbp_search(raw_t, pos_plat, vel_plat, t_start, num_samples, vel_hyps, t_pulses, scene_size, nx, ny, *, images=False,
                consts=None, ctx=None, chunks=None):
    """Back-projection of one CPI under every focus velocity of ``vel_hyps`` [n_hyp x 3] in one enqueue (arguments as
    ``tdbp_gpu``, whose plan cache is shared).  raw_t: NumPy array or the DeviceBuffer of run_physics_spotlight(device=True).
    ``images=True`` also returns the stack.  ``chunks``: pulse chunks (None = chosen by the library)."""
    k = consts or batch_constants()
    ctx = ctx or default_context()
    hyp = _host.hypotheses(vel_hyps)
    n_hyp, n_p = hyp.shape[0], len(t_pulses)
    plan = cached_plan(ctx, k, n_p, num_samples, nx, ny)
    nx, ny = int(nx), int(ny)
    pos, vel, tp, _ = _host.geometry(n_p, pos_plat, vel_plat, t_pulses)
    lib = ctx.lib
    _host.set_chunks(plan, chunks)
    rec = np.zeros(max(n_hyp, 1), dtype=RECORD_DTYPE)
    stack = None
    if isinstance(raw_t, DeviceBuffer):
        bufs = plan._d_search
        if "rec" not in bufs:
            bufs["rec"] = ctx.alloc(_ffi.TDBP_SEARCH_MAX_HYP * RECORD_DTYPE.itemsize)
        d_img = None
        images = images and 1 <= n_hyp <= _ffi.TDBP_SEARCH_MAX_HYP      # a bad n_hyp sizes nothing: the library refuses it below
        if images:
            need = n_hyp * ny * nx * 16
            if "img" not in bufs or bufs["img"].nbytes < need:
                if "img" in bufs:
                    bufs.pop("img").release()
                bufs["img"] = ctx.alloc(need)
            d_img = bufs["img"]
        check(lib.sarx_tdbp_search_dev(plan.h, raw_t.ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t_start),
                                       hyp.ctypes.data, n_hyp, float(scene_size), d_img.ptr if images else None, bufs["rec"].ptr), ctx.h)
        rec = bufs["rec"].download(np.uint8, (n_hyp * RECORD_DTYPE.itemsize,)).view(RECORD_DTYPE).copy()
        if images:
            stack = d_img.download(np.complex128, (n_hyp, ny, nx))
    else:
        x = np.ascontiguousarray(raw_t, dtype=np.complex64)
        if x.shape != (n_p, int(num_samples)):
            raise ValueError(f"raw must be [{n_p} x {int(num_samples)}]")
        if images and 1 <= n_hyp <= _ffi.TDBP_SEARCH_MAX_HYP:
            stack = np.empty((n_hyp, ny, nx), dtype=np.complex128)
        check(lib.sarx_tdbp_search_host(plan.h, x.ctypes.data, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t_start),
                                        hyp.ctypes.data, n_hyp, float(scene_size), stack.ctypes.data if stack is not None else None,
                                        rec.ctypes.data), ctx.h)
        rec = rec[:n_hyp]
    return TdbpSearchResult(hyp.copy(), rec, stack, _host.route(lib.sarx_tdbp_search_route, plan))


def tdbp_autofocus(raw_t, pos_plat, vel_plat, t_start, num_samples, t_pulses, scene_size, nx, ny, *, v0, half_span, n,
                   direction=None, metric="s4", consts=None, ctx=None, d_image=None, pga=None, pga_axis=0):
    """One search on the line ``v0 + s * direction`` (n odd hypotheses over +-half_span; direction defaults to the ground
    projection of the mean platform velocity: the along-track direction, the only component sharpness can tell) and one
    ``tdbp_gpu`` at the estimate.  returns (v_est [3], image complex128 [ny x nx], TdbpSearchResult).  v0 carries what is known
    from elsewhere - the radial component above all.  ``d_image`` as in ``tdbp_gpu`` (device input only): the image is left there
    and None is returned in its place.  ``pga``: a PgaParams: the frame at the estimate is passed through ``sarx.pga`` (as
    complex64, azimuth along image axis ``pga_axis``; 1 needs nx and ny to be multiples of 32) before it is returned, which removes
    what no velocity can: a phase error over the aperture that is not a parabola.  It needs the host image (no ``d_image``)."""
    if pga is not None and d_image is not None:
        raise ValueError("pga takes the host image: d_image holds complex128, the autofocus works on complex64")
    if direction is None:
        direction = np.asarray(vel_plat, dtype=np.float64).mean(axis=0) * np.array([1.0, 1.0, 0.0])
    hyps = tdbp_velocity_line(v0, direction, half_span, n)
    res = tdbp_search(raw_t, pos_plat, vel_plat, t_start, num_samples, hyps, t_pulses, scene_size, nx, ny, consts=consts, ctx=ctx)
    v_est = res.estimate(metric).velocity
    img = tdbp_gpu(raw_t, pos_plat, vel_plat, t_start, num_samples, v_est, t_pulses, scene_size, nx, ny, consts=consts, ctx=ctx,
                   d_image=d_image)
    if pga is not None:
        from .pga import pga as _pga
        img = _pga(np.asarray(img, dtype=np.complex64), pga, axis=pga_axis, ctx=ctx).image.astype(np.complex128)
    return v_est, img, res
