"""Ground relocation of GMTI reports on the device (include/sarx_relocate.h).

A mover is imaged at the ground point whose range and range rate match its own, hundreds of metres along track from where it is.
``ground_relocate`` takes a report list on a back-projection's ground grid and one radial speed per report (the pair's ATI speed,
the resolver's ``v_los``) and gives each report the ground position at the same range whose range rate is less by that speed.  The
relocated reports are a GMTI slot again, on an output grid of the caller's choosing: the tracker and the plot extraction take it
unchanged, in ground coordinates.  ``relocate_frames`` does so for the frames of a VideoSAR run, into the stack ``track.enqueue_run``
reads.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi, _tdbp_host as _host, slot as _slot
from ._ffi import check
from .engine import default_context

RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("shift_x", "<f8"), ("shift_y", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("rank", "<i4"),
                         ("status", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert RECORD_DTYPE.itemsize == C.sizeof(_ffi.RelocateRecord) == 64 and C.sizeof(_ffi.RelocateParams) == 128


def reference_geometry(pos_tx, vel_tx, t_pulses, rx_offsets=(0.0, 0.0)):
    """(pos_ref, vel_ref) of a CPI imaged from the channel pair at ``rx_offsets`` = (off_a, off_b): the pair's mean phase centre and
    its velocity at the reference time mean(t_pulses), the dt = 0 of sarx_tdbp_*.

    pos_tx and vel_tx are interpolated linearly at that time.  Receiver c rides at pos_tx + off_c unit(vel_tx), and the two-way path
    |g - p_tx| + |g - p_rx| is twice the distance to the point midway between transmitter and receiver: channel c's phase centre
    lies off_c / 2 ahead of the transmitter (the rule of the pair's lag, (off_b - off_a) / (2 V)), the mean of the two channels'
    (off_a + off_b) / 4 ahead.  That, not (off_a + off_b) / 2, is taken here."""
    pos = np.asarray(pos_tx, dtype=np.float64)
    vel = np.asarray(vel_tx, dtype=np.float64)
    tp = np.asarray(t_pulses, dtype=np.float64)
    off = np.asarray(rx_offsets, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or vel.shape != pos.shape or tp.shape != (len(pos),) or off.shape != (2,):
        raise ValueError("pos_tx and vel_tx must be [n_pulses x 3], t_pulses [n_pulses], rx_offsets (off_a, off_b)")
    if len(tp) > 1 and not np.all(np.diff(tp) > 0):
        raise ValueError("t_pulses must rise")
    t0 = float(np.mean(tp))
    p = np.array([np.interp(t0, tp, pos[:, k]) for k in range(3)])
    v = np.array([np.interp(t0, tp, vel[:, k]) for k in range(3)])
    speed = float(np.linalg.norm(v))
    if not speed > 0:
        raise ValueError("the platform does not move at the reference time")
    return p + 0.5 * (0.5 * (off[0] + off[1])) * v / speed, v


def grid_of(grid):
    """(x0, y0, dx, dy, nx, ny) of a ``tdbp_gpu`` grid (scene_size, nx, ny): linspace(-S / 2, S / 2, n) per axis."""
    size, nx, ny = float(grid[0]), int(grid[1]), int(grid[2])
    if nx < 1 or ny < 1:
        raise ValueError("grid = (scene_size, nx, ny) with nx, ny >= 1")
    return (-size / 2, -size / 2, size / (nx - 1) if nx > 1 else size, size / (ny - 1) if ny > 1 else size, nx, ny)


def relocate_params(pos_ref, vel_ref, grid, out_grid, max_detections):
    """The sarx_relocate_params block; grid (scene_size, nx, ny), out_grid (x0, y0, dx, dy, nx, ny) or None = the input grid."""
    pos, vel = np.asarray(pos_ref, dtype=np.float64), np.asarray(vel_ref, dtype=np.float64)
    if pos.shape != (3,) or vel.shape != (3,):
        raise ValueError("pos_ref and vel_ref must be [3]")
    gin = grid_of(grid)
    out = gin if out_grid is None else tuple(out_grid)
    if len(out) != 6:
        raise ValueError("out_grid = (x0, y0, dx, dy, nx, ny)")
    return _ffi.RelocateParams((C.c_double * 3)(*pos), (C.c_double * 3)(*vel), *(float(x) for x in gin[:4]), *(float(x) for x in out[:4]),
                               int(out[4]), int(out[5]), int(max_detections), 0)


def _is_device_pair(x):
    return isinstance(x, tuple) and len(x) == 2 and (hasattr(x[0], "ptr") or isinstance(x[0], int))


def _per_report(ctx, x, dtype, md, held, what):
    """(address, stride) of a per-report input: a host array (uploaded into ``held``, padded to md elements) or a
    (DeviceArray / address, stride) pair that lies on the device already; (None, 0) for None."""
    if x is None:
        return None, 0
    if _is_device_pair(x):
        return (x[0].ptr if hasattr(x[0], "ptr") else int(x[0])), int(x[1])
    a = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    if len(a) > md:
        raise ValueError(f"{what}: {len(a)} values for a slot of {md} reports")
    full = np.zeros(md, dtype)
    full[:len(a)] = a
    return _host.hold(held, ctx.to_device(full)).ptr, full.itemsize


def enqueue(ctx, prm, slot_ptr, v_los, valid, v_along, records_ptr, out_slot_ptr):
    """The two launches on the ctx's current lane; only enqueues.  v_los, valid, v_along: (address or None, stride)."""
    check(ctx.lib.sarx_relocate_dev(ctx.h, C.byref(prm), slot_ptr, v_los[0], v_los[1], valid[0], valid[1], v_along[0], v_along[1], records_ptr,
                                    out_slot_ptr), ctx.h)


class RelocateResult:
    """``records``: one per input report (RECORD_DTYPE: x, y, shift_x, shift_y, vx, vy, rank, status, flags); ``slot``: the output
    slot's bytes (header and kept reports); ``reports``: its report array (slot.REPORT_DTYPE, sorted by output pixel);
    ``x``, ``y``, ``status``: the records' columns."""

    def __init__(self, records, slot):
        self.records, self.slot = records, slot
        self.reports = _slot.reports(slot).copy()
        self.x, self.y, self.status = records["x"], records["y"], records["status"]

    def __len__(self):
        return len(self.records)

    def __repr__(self):
        return f"RelocateResult({len(self.records)} reports, {len(self.reports)} kept)"


def ground_relocate(reports, v_los, *, pos_ref, vel_ref, grid, out_grid=None, valid=None, v_along=None, max_detections=None, ctx=None):
    """Each report of a list on the ground grid ``grid`` = (scene_size, nx, ny) of ``tdbp_gpu`` moved to where its mover is.

    reports  : a GmtiReport, a REPORT_DTYPE array, a slot's bytes, or a device slot (anything with .ptr, with ``max_detections`` =
               its capacity); i = row (y), j = column (x) of the image
    v_los    : radial speed per report, m/s, receding positive (TdbpPairResult.v_los, the resolver's record): a host array, or
               (DeviceArray / address, stride in bytes) of values on the device - the resolver's records go in as
               ``v_los=(rec, 64), valid=(rec.ptr + 60, 64)``
    valid    : uint32 per report, non-zero = the report has no speed (the resolver's status); host array, device pair or None
    v_along  : the target's ground speed along the track direction per report (NaN = none), for the ground velocity; or None
    pos_ref, vel_ref : the phase centre and its velocity at the CPI's reference time (``reference_geometry``)
    out_grid : (x0, y0, dx, dy, nx, ny) of the output slot's pixels, None = the input grid
    Returns a RelocateResult; raises GmtiOverflowError on an overflowed slot."""
    ctx = ctx or default_context()
    md, stack, on_device = _slot.stage(reports, max_detections=max_detections, single=True)
    prm = relocate_params(pos_ref, vel_ref, grid, out_grid, md)
    check(ctx.lib.sarx_relocate_check(C.byref(prm)))
    if not on_device:                                      # a host list tells its length: a host array must speak for every report
        n, overflowed = _slot.header(stack[0])
        for name, x in (("v_los", v_los), ("valid", valid), ("v_along", v_along)):
            if x is not None and not _is_device_pair(x) and np.size(x) != n and n <= md and not overflowed:
                raise ValueError(f"{name}: {np.size(x)} values for {n} reports")
    with _host.temporaries() as held:
        p_slot = _host.slot_on_device(ctx, stack, on_device, held)
        speeds = _per_report(ctx, v_los, np.float64, md, held, "v_los")
        if speeds[0] is None:
            raise ValueError("v_los is needed: one radial speed per report")
        flags = _per_report(ctx, valid, np.uint32, md, held, "valid")
        along = _per_report(ctx, v_along, np.float64, md, held, "v_along")
        rec = _host.hold(held, ctx.alloc(md * RECORD_DTYPE.itemsize))
        out = _host.hold(held, ctx.alloc(_slot.slot_bytes(md)))
        enqueue(ctx, prm, p_slot, speeds, flags, along, rec.ptr, out.ptr)
        count = _slot.raise_if_overflowed(*_slot.header(_slot.fetch_header(ctx, p_slot)), md, strict=True)
        records = _slot.download(ctx, rec.ptr, count * RECORD_DTYPE.itemsize).view(RECORD_DTYPE).copy()
        return RelocateResult(records, _slot.fetch(ctx, out.ptr, md))


def relocate_frames(ctx, slots, v_los, *, geometry, grid, out_grid=None, valid=None, v_along=None, max_detections, stack=None, records=None):
    """One ``sarx_relocate_dev`` per frame, enqueued on the ctx's current lane into ONE stack of output slots
    ``slot.slot_bytes(max_detections)`` apart (the tracker's TrackParams.slot_bytes()), so that ``track.enqueue_run`` takes it.

    slots    : per frame a device slot (anything with .ptr) of capacity max_detections
    v_los, valid, v_along : per frame a (DeviceArray / address, stride) pair (valid, v_along: or None for all frames)
    geometry : per frame (pos_ref, vel_ref)
    stack, records : device buffers to write into (n_frames slots; n_frames x max_detections records), made here when None
    Returns (stack, records), both on the device and the caller's to release; nothing is waited for."""
    n, md = len(slots), int(max_detections)
    if not (len(v_los) == len(geometry) == n) or any(x is not None and len(x) != n for x in (valid, v_along)):
        raise ValueError("one entry per frame")
    stride = _slot.slot_bytes(md)
    stack = stack or ctx.alloc(max(n, 1) * stride)
    records = records or ctx.alloc(max(n, 1) * md * RECORD_DTYPE.itemsize)
    none = (None, 0)
    if any(x is not None and not all(_is_device_pair(y) for y in x) for x in (v_los, valid, v_along)):
        raise TypeError("relocate_frames takes (DeviceArray / address, stride) pairs; host arrays go through ground_relocate")
    for f in range(n):
        prm = relocate_params(geometry[f][0], geometry[f][1], grid, out_grid, md)
        pairs = [none if x is None else _per_report(ctx, x[f], None, md, None, "device pair") for x in (v_los, valid, v_along)]
        enqueue(ctx, prm, slots[f].ptr, *pairs, records.ptr + f * md * RECORD_DTYPE.itemsize, stack.ptr + f * stride)
    return stack, records
