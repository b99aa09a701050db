"""The host work that the back-projection wrappers (tdbp, tdbp_search, tdbp_pair, tdbp_pair_search, tdbp_multi) share, each rule
once: what happens to their arguments before a C entry point sees them and to its answer afterwards."""
import contextlib
import ctypes as C

import numpy as np

from ._ffi import check
from .engine import DeviceArray, DeviceBuffer

C64, C128 = np.dtype(np.complex64), np.dtype(np.complex128)


def geometry(n_p, pos, vel, t_pulses, vel_focus=None):
    """One CPI's geometry as contiguous fp64: (pos, vel [n_pulses x 3], t_pulses [n_pulses], vel_focus [3] or None)."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    tp = np.ascontiguousarray(t_pulses, dtype=np.float64)
    vf = None if vel_focus is None else np.ascontiguousarray(vel_focus, dtype=np.float64)
    if pos.shape != (n_p, 3) or vel.shape != (n_p, 3) or tp.shape != (n_p,) or (vf is not None and vf.shape != (3,)):
        raise ValueError("platform positions and velocities must be [n_pulses x 3], t_pulses [n_pulses], vel_focus [3]")
    return pos, vel, tp, vf


def hypotheses(vel_hyps):
    hyp = np.ascontiguousarray(vel_hyps, dtype=np.float64)
    if hyp.ndim != 2 or hyp.shape[1] != 3:
        raise ValueError("vel_hyps must be [n_hyp x 3]")
    return hyp


def raw_ptr(x, n_p, n_s, keep):
    """(address, on the device?) of one channel's [n_p x n_s] complex64 samples; a host array is made contiguous and kept in ``keep``."""
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


def raw_ptrs(raws, n_p, n_s):
    """(addresses, on the device?, the host arrays to keep alive) of every channel: all host arrays or all device-resident."""
    keep = []
    found = [raw_ptr(r, n_p, n_s, keep) for r in raws]
    if any(dev != found[0][1] for _, dev in found):
        raise ValueError("the raw arrays must all be host arrays or all device-resident")
    return [p for p, _ in found], found[0][1], keep


def raw_on_device(ctx, raws, n_p, n_s, held):
    """Device addresses of every channel for an entry point that reads the device only: a host array is uploaded into ``held``."""
    ptrs, keep = [], []
    for raw in raws:
        p, dev = raw_ptr(raw, n_p, n_s, keep)
        ptrs.append(p if dev else hold(held, ctx.to_device(keep[-1])).ptr)
    return ptrs


def slot_on_device(ctx, stack, on_device, held):
    """Address of the one slot that slot.stage(single=True) staged: the caller's device slot, or the host one uploaded into ``held``."""
    return on_device[0][1] if on_device else hold(held, ctx.to_device(stack[0])).ptr


@contextlib.contextmanager
def temporaries():
    """A list of device buffers that are released, in the order they were taken, however the block is left."""
    held = []
    try:
        yield held
    finally:
        for b in held:
            b.release()


def hold(held, buf):
    held.append(buf)
    return buf


def route(fn, plan):
    """What a ``sarx_tdbp_*_route`` query says of the plan's last launch: "tile" or "exact"."""
    tile = C.c_int()
    check(fn(plan.h, C.byref(tile)), plan.ctx.h)
    return "tile" if tile.value else "exact"


def mean_speed(vel):
    return float(np.mean(np.linalg.norm(np.asarray(vel, dtype=np.float64), axis=1)))


def lags(rx_offsets, vel):
    """Per baseline (0, b): the phase centres (midway between transmitter and receiver) lie (off_b - off_0) / 2 apart along track, so
    channel b's passes a point this much later (with offsets -+ V / PRF and the DPCA pulse shift: exactly one pulse interval)."""
    off = np.asarray(rx_offsets, dtype=np.float64)
    return (off[1:] - off[0]) / (2.0 * mean_speed(vel))


def chirp_centre(consts, chirp_centre):
    """None = T_P / 2: the chirp of run_bistatic_physics_gpu starts at the delay."""
    return consts["T_P"] / 2 if chirp_centre is None else chirp_centre


def set_chunks(plan, chunks):
    """The plan's pulse-chunk count, which serves every launch on it (None = chosen by the library)."""
    check(plan.ctx.lib.sarx_tdbp_search_set_chunks(plan.h, 0 if chunks is None else int(chunks)), plan.ctx.h)


def focus_channels(e_check, e_dev, e_host, e_route, params_of, pass_raw, plan_of, ctx, consts, raws, pos_tx, vel_tx, rx_offsets, t_start,
                   num_samples, t_pulses, scene_size, nx, ny, vel_focus, centre, device_output, dtype, chunks):
    """The body of ``tdbp_pair`` and ``tdbp_multi``: n_rx channels of one CPI through the family's check, dev, host and route entry
    points ``e_*``.  ``params_of(n_p, off, vel, tp, centre)`` builds its parameter block, ``pass_raw(addresses)`` the arguments
    that carry the raw pointers, ``plan_of`` is tdbp.cached_plan.  Returns (stack, lags, route): the stack a NumPy array
    [n_rx x ny x nx], or with ``device_output`` the complex64 DeviceBuffer that holds it, the caller's from then on."""
    n_p, n_s, nx, ny = len(t_pulses), int(num_samples), int(nx), int(ny)
    dtype = np.dtype(dtype or (C64 if device_output else C128))
    if dtype not in (C64, C128) or (device_output and dtype != C64):
        raise ValueError("dtype must be complex128 or complex64 (complex64 with device_output)")
    pos, vel, tp, vf = geometry(n_p, pos_tx, vel_tx, t_pulses, vel_focus)
    off = np.asarray(rx_offsets, dtype=np.float64)
    n_rx = len(raws)
    if off.shape != (n_rx,):
        raise ValueError("one raw array per receiver offset")
    prm = params_of(n_p, off, vel, tp, chirp_centre(consts, centre))
    check(e_check(n_p, C.byref(prm)))
    plan = plan_of(ctx, consts, n_p, n_s, nx, ny)
    ptrs, on_device, keep = raw_ptrs(raws, n_p, n_s)            # keep: alive until the launch has returned
    if device_output and not on_device:
        raise ValueError("device_output needs device-resident raw")
    args = (plan.h, *pass_raw(ptrs), pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, float(t_start), vf.ctypes.data, float(scene_size),
            C.byref(prm))
    wide = dtype == C128
    set_chunks(plan, chunks)
    if on_device:
        with temporaries() as held:
            stack = hold(held, ctx.alloc(n_rx * ny * nx * dtype.itemsize))
            check(e_dev(*args, stack.ptr if wide else None, None if wide else stack.ptr), ctx.h)
            if device_output:
                held.clear()                       # launched: the buffer is the caller's
            else:
                stack = stack.download(dtype, (n_rx, ny, nx))
    else:
        stack = np.empty((n_rx, ny, nx), dtype=dtype)
        check(e_host(*args, stack.ctypes.data if wide else None, None if wide else stack.ctypes.data), ctx.h)
    return stack, lags(off, vel), route(e_route, plan)
