"""Ground tracking of relocated GMTI reports on the GPU: a Kalman filter per track that uses the radial speed (include/sarx_ktrack.h,
csrc/ktrack.hip).

A relocated report's position error is an ellipse along the track direction (R / |V_xy| seconds of along-track shift per m/s of
speed error) that turns with the aspect angle, it is correlated with the error of v_los, and v_los itself measures one component of
the ground velocity.  Each track carries (x, y, vx, vy) in metres and m/s with its 4 x 4 covariance; a report is gated on the
Mahalanobis distance of (x, y, v_los), tracks and reports are tied by one round of mutual nearest neighbour, and a new track starts
with the velocity component its first report measures.  Confirmation (M of N), drops, births and the overflow rules are those of
sarx.track.  The input of a step is what ONE ground relocation read and wrote: its input slot, its records and its v_los array, left
on the device.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _ffi, _tdbp_host as _host, slot as _slot
from ._ffi import SarxError, check
from .relocate import RECORD_DTYPE, _is_device_pair, _per_report
from .slot import GmtiOverflowError
from .track import TrackOverflowError

HEADER_BYTES = C.sizeof(_ffi.KtrackHeader)
HEADER_DTYPE = np.dtype([("n_live", "<u4"), ("n_confirmed", "<u4"), ("next_id", "<i4"), ("frames_done", "<u4"), ("births_total", "<u4"),
                         ("drops_total", "<u4"), ("error", "<u4"), ("error_frame", "<i4"), ("max_tracks", "<u4"), ("reserved0", "<u4"),
                         ("t_last", "<f8"), ("reserved", "<u4", (4,))])
SLOT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("p", "<f8", (10,)), ("sum_re", "<f8"), ("sum_im", "<f8"),
                       ("sum_power", "<f8"), ("max_ratio", "<f8"), ("nis_last", "<f8"), ("nis_sum", "<f8"), ("id", "<i4"), ("status", "<u4"),
                       ("hits", "<u4"), ("misses", "<u4"), ("age", "<u4"), ("hist", "<u4"), ("last_frame", "<i4"), ("last_report", "<i4")])
TRACK_DTYPE = np.dtype([("id", "<i4"), ("slot", "<i4"), ("status", "<u4"), ("confirmed", "?"), ("x", "<f8"), ("y", "<f8"), ("vx", "<f8"),
                        ("vy", "<f8"), ("speed", "<f8"), ("heading", "<f8"), ("cov", "<f8", (4, 4)), ("hits", "<u4"), ("misses", "<u4"),
                        ("age", "<u4"), ("last_frame", "<i4"), ("last_report", "<i4"), ("nis_last", "<f8"), ("nis_mean", "<f8"),
                        ("interf", "<c16"), ("sum_power", "<f8"), ("max_ratio", "<f8")])
assert HEADER_DTYPE.itemsize == HEADER_BYTES == 64 and SLOT_DTYPE.itemsize == C.sizeof(_ffi.KtrackSlot) == 192
_TRIANGLE = [(i, j) for i in range(4) for j in range(i, 4)]           # the order of sarx_ktrack_slot.p


class TrackTimeError(SarxError):
    """The tracker stopped at `frame`: its time lies before the previous step's (or the difference is not finite)."""

    def __init__(self, frame):
        super().__init__(-1, f"ground tracker: the time of frame {frame} lies before the previous step's")
        self.frame = int(frame)


@dataclass
class KalmanTrackParams:
    """sigma_pos (m): placement error of a report per axis; sigma_v (m/s): error of v_los; sigma_v_tan (m/s): prior of the velocity
    component a first report does not measure; q (m^2/s^3): white-acceleration density; gate_d2: gate on the Mahalanobis distance
    squared of (x, y, v_los), 3 degrees of freedom (16.27 holds 99.9 %); gate_m (m): half-width of the coarse box on the position
    innovation, part of the decision; confirm = (M, N), max_misses, birth_ratio, max_tracks: as sarx.TrackParams; max_detections:
    capacity of the slots, records and v_los arrays."""
    sigma_pos: float = 1.0
    sigma_v: float = 0.3
    sigma_v_tan: float = 10.0
    q: float = 0.01
    gate_d2: float = 16.27
    gate_m: float = 100.0
    confirm: Tuple[int, int] = (3, 5)
    max_misses: int = 3
    birth_ratio: float = 0.0
    max_tracks: int = 1024
    max_detections: int = 4096

    def check(self):
        try:
            m, n = (int(x) for x in self.confirm)
        except (TypeError, ValueError):
            raise ValueError("confirm must be (M, N)") from None
        for name in ("sigma_pos", "sigma_v", "sigma_v_tan", "gate_d2", "gate_m"):
            v = float(getattr(self, name))
            if not (v > 0 and math.isfinite(v)):
                raise ValueError(f"{name} must be finite and > 0")
        for name in ("q", "birth_ratio"):
            v = float(getattr(self, name))
            if not (v >= 0 and math.isfinite(v)):
                raise ValueError(f"{name} must be finite and >= 0")
        if not 1 <= m <= n <= 32:
            raise ValueError("confirm = (M, N) needs 1 <= M <= N <= 32")
        if int(self.max_misses) < 0:
            raise ValueError("max_misses must be >= 0")
        if not 1 <= int(self.max_tracks) <= _ffi.KTRACK_MAX_TRACKS:
            raise ValueError(f"max_tracks must be 1 .. {_ffi.KTRACK_MAX_TRACKS}")
        if not 1 <= int(self.max_detections) <= _ffi.KTRACK_MAX_DETECTIONS:
            raise ValueError(f"max_detections must be 1 .. {_ffi.KTRACK_MAX_DETECTIONS}")
        return m, n

    def c_params(self):
        m, n = self.check()
        return _ffi.KtrackParams(float(self.sigma_pos), float(self.sigma_v), float(self.sigma_v_tan), float(self.q), float(self.gate_d2),
                                 float(self.gate_m), float(self.birth_ratio), m, n, int(self.max_misses), int(self.max_tracks),
                                 int(self.max_detections), 0)

    def slot_bytes(self):
        return _slot.slot_bytes(self.max_detections)


def c_frame(t, pos_ref, vel_ref, frame_index):
    """The sarx_ktrack_frame block of one step."""
    pos, vel = np.asarray(pos_ref, dtype=np.float64), np.asarray(vel_ref, dtype=np.float64)
    if pos.shape != (3,) or vel.shape != (3,):
        raise ValueError("pos_ref and vel_ref must be [3]")
    return _ffi.KtrackFrame(float(t), (C.c_double * 3)(*pos), (C.c_double * 3)(*vel), int(frame_index), 0)


def table_bytes(cp):
    n = C.c_size_t()
    check(_ffi.load().sarx_ktrack_table_bytes(C.byref(cp), C.byref(n)))
    return n.value


def workspace_bytes(cp):
    n = C.c_size_t()
    check(_ffi.load().sarx_ktrack_workspace_bytes(C.byref(cp), C.byref(n)))
    return n.value


def enqueue_init(ctx, cp, table_ptr):
    check(ctx.lib.sarx_ktrack_init_dev(ctx.h, C.byref(cp), table_ptr), ctx.h)


def enqueue_step(ctx, cp, frame, slot_ptr, records_ptr, v_los, table_ptr, assoc_ptr, workspace_ptr):
    """One step's launches on the ctx's current lane; only enqueues.  frame: c_frame(...); v_los: (address, stride in bytes)."""
    check(ctx.lib.sarx_ktrack_step_dev(ctx.h, C.byref(cp), C.byref(frame), slot_ptr, records_ptr, v_los[0], int(v_los[1]), table_ptr, assoc_ptr,
                                       workspace_ptr), ctx.h)


def enqueue_run(ctx, cp, frames, slots, records, v_los, table_ptr, assoc_ptr, workspace_ptr):
    """Every frame of `frames` (a list of c_frame blocks) over slots = (address, stride), records = (address, stride) and v_los =
    (address, stride between reports, stride between frames), all strides in bytes; only enqueues."""
    arr = (_ffi.KtrackFrame * max(len(frames), 1))(*frames)
    check(ctx.lib.sarx_ktrack_run_dev(ctx.h, C.byref(cp), arr, len(frames), slots[0], int(slots[1]), records[0], int(records[1]), v_los[0],
                                      int(v_los[1]), int(v_los[2]), table_ptr, assoc_ptr, workspace_ptr), ctx.h)


class KalmanTrackResult:
    """`tracks`: the live table decoded (TRACK_DTYPE, rising slot index): id, status, x, y, vx, vy, speed = |v|, heading = atan2(vy,
    vx) in degrees, cov (4 x 4, symmetric), hits, nis_mean = nis_sum / (hits - 1) (NaN before the second hit) ...; `confirmed`: the
    rows of `tracks` that are confirmed; `header`; `assoc` [n_frames x max_detections] int32 (track id per input report, -1 =
    none); `raw`: the table's bytes.  Raises what the table's error field says: TrackTimeError, else TrackOverflowError (kind "slot"
    or "table"; GroundTracker.result turns "slot" into the GmtiOverflowError of the frame's list)."""

    def __init__(self, raw, assoc):
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self.raw, self.assoc = raw, np.asarray(assoc, np.int32)
        self.header = raw[:HEADER_BYTES].view(HEADER_DTYPE)[0]
        err, frame = int(self.header["error"]), int(self.header["error_frame"])
        if err == _ffi.KTRACK_ERR_TIME:
            raise TrackTimeError(frame)
        if err != _ffi.KTRACK_OK:
            raise TrackOverflowError(err, frame)
        slots = raw[HEADER_BYTES:].view(SLOT_DTYPE)
        live = np.flatnonzero(slots["status"] != _ffi.KTRACK_FREE)
        s = slots[live]
        t = np.zeros(len(live), TRACK_DTYPE)
        t["slot"], t["confirmed"] = live, s["status"] == _ffi.KTRACK_CONFIRMED
        for k in ("id", "status", "x", "y", "vx", "vy", "hits", "misses", "age", "last_frame", "last_report", "nis_last", "sum_power", "max_ratio"):
            t[k] = s[k]
        t["speed"] = np.hypot(s["vx"], s["vy"])
        t["heading"] = np.degrees(np.arctan2(s["vy"], s["vx"]))
        for k, (i, j) in enumerate(_TRIANGLE):
            t["cov"][:, i, j] = t["cov"][:, j, i] = s["p"][:, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            t["nis_mean"] = np.where(s["hits"] > 1, s["nis_sum"] / (s["hits"].astype(np.float64) - 1.0), np.nan)
        t["interf"] = s["sum_re"] + 1j * s["sum_im"]
        self.tracks = t
        self.confirmed = t[t["confirmed"]]
        self.n_live, self.n_confirmed = int(self.header["n_live"]), int(self.header["n_confirmed"])

    def __repr__(self):
        return f"KalmanTrackResult({self.n_live} live, {self.n_confirmed} confirmed over {len(self.assoc)} frames)"


class GroundTracker:
    """A Kalman track table on the device.  step() enqueues one frame and never waits; result() downloads table and assoc."""

    def __init__(self, ctx, params, max_frames=256):
        self.ctx, self.params, self.max_frames = ctx, params, int(max_frames)
        self.cp = params.c_params()
        self.table = ctx.alloc(table_bytes(self.cp))
        self.ws = ctx.alloc(workspace_bytes(self.cp))
        self.d_assoc = ctx.alloc(self.max_frames * params.max_detections * 4)
        self._own = []
        self._slots = []                     # per frame: the address of its slot, for the count of one that overflowed
        self.n_steps = 0
        enqueue_init(ctx, self.cp, self.table.ptr)

    def step(self, slot, records, v_los, *, pos_ref, vel_ref, t):
        """slot: the relocation's INPUT slot - a device slot (anything with .ptr, left alone until result()) or host data (GmtiReport,
        report array, slot bytes; uploaded); records: its sarx_relocate_record array - (DeviceArray / address, stride) or a host
        RECORD_DTYPE array; v_los: (DeviceArray / address, stride) or a host array; pos_ref, vel_ref: what that relocation was given;
        t: the frame's time in seconds.  Returns the frame's index."""
        f, md = self.n_steps, self.params.max_detections
        if f >= self.max_frames:
            raise ValueError(f"more than max_frames={self.max_frames} steps")
        frame = c_frame(t, pos_ref, vel_ref, f)
        _, stack, on_device = _slot.stage(slot, max_detections=md, single=True)
        p_slot = _host.slot_on_device(self.ctx, stack, on_device, self._own)
        if _is_device_pair(records):
            if int(records[1]) != RECORD_DTYPE.itemsize:
                raise ValueError(f"records lie {RECORD_DTYPE.itemsize} bytes apart")
            p_rec = records[0].ptr if hasattr(records[0], "ptr") else int(records[0])
        else:
            rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE).reshape(-1)
            if len(rec) > md:
                raise ValueError(f"records: {len(rec)} for a slot of {md} reports")
            full = np.zeros(md, RECORD_DTYPE)
            full[:len(rec)] = rec
            p_rec = _host.hold(self._own, self.ctx.to_device(full)).ptr
        speeds = _per_report(self.ctx, v_los, np.float64, md, self._own, "v_los")
        if speeds[0] is None:
            raise ValueError("v_los is needed: one radial speed per report")
        enqueue_step(self.ctx, self.cp, frame, p_slot, p_rec, speeds, self.table.ptr, self.d_assoc.ptr + f * md * 4, self.ws.ptr)
        self._slots.append(p_slot)
        self.n_steps += 1
        return f

    def result(self):
        """Waits for the steps enqueued so far.  Raises TrackOverflowError (a full table), GmtiOverflowError (an overflowed report
        list) or TrackTimeError if the table holds an error."""
        md = self.params.max_detections
        raw = self.table.download(np.uint8, (self.table.nbytes,))
        assoc = self.d_assoc.download(np.int32, (self.max_frames, md))[:self.n_steps].copy()
        hdr = raw[:HEADER_BYTES].view(HEADER_DTYPE)[0]
        if int(hdr["error"]) == _ffi.KTRACK_ERR_SLOT_OVERFLOW and 0 <= int(hdr["error_frame"]) < len(self._slots):
            count, _ = _slot.header(_slot.fetch_header(self.ctx, self._slots[int(hdr["error_frame"])]))
            raise GmtiOverflowError(count, md)
        return KalmanTrackResult(raw, assoc)

    def close(self):
        for b in (self.table, self.ws, self.d_assoc, *self._own):
            b.release()
        self._own = []


def ground_track(slots, records, v_los, *, geometry, times, params=None, ctx=None):
    """Track the frames of a VideoSAR run over what ``relocate_frames`` read and wrote.

    slots    : per frame the relocation's INPUT slot: a device slot (anything with .ptr) or host data
    records  : the record stack ``relocate_frames`` returned (a DeviceArray / buffer of n_frames x max_detections records), or per
               frame a host RECORD_DTYPE array
    v_los    : per frame a (DeviceArray / address, stride) pair or a host array: what the relocation read
    geometry : per frame (pos_ref, vel_ref), as given to ``relocate_frames``;  times: per frame t in seconds
    Returns a KalmanTrackResult; raises TrackOverflowError, GmtiOverflowError or TrackTimeError."""
    from .engine import default_context
    params = params or KalmanTrackParams()
    n = len(slots)
    if not (len(v_los) == len(geometry) == len(times) == n):
        raise ValueError("one entry per frame")
    stacked = hasattr(records, "ptr")
    if not stacked and len(records) != n:
        raise ValueError("one entry per frame")
    ctx = ctx or default_context()
    md = params.max_detections
    trk = GroundTracker(ctx, params, max_frames=max(n, 1))
    try:
        for f in range(n):
            rec = (records.ptr + f * md * RECORD_DTYPE.itemsize, RECORD_DTYPE.itemsize) if stacked else records[f]
            trk.step(slots[f], rec, v_los[f], pos_ref=geometry[f][0], vel_ref=geometry[f][1], t=times[f])
        return trk.result()
    finally:
        trk.close()
