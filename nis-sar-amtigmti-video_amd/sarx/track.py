"""GMTI tracking on the GPU: the report lists of consecutive frames tied into tracks with one id per mover, false alarms that do
not persist dropped by an M-of-N rule, and the ATI speed unwrapped with the track's range rate (include/sarx_track.h,
csrc/track.hip).

Semantics (the kernels implement them; include/sarx_track.h states them step by step):
  A track is a position and a velocity in pixels (i = azimuth row, j = range column) and pixels per frame.  Per frame: predict
  p + v; a report is eligible for a track when ((i - p_i) / gate_az)^2 + ((j - p_j) / gate_rg)^2 <= 1; track and report are matched
  when each is the other's nearest eligible partner (one round of mutual nearest neighbour - a track whose best report prefers
  another track coasts); a matched track moves by alpha (position) and beta (velocity) times the innovation.  A tentative track is
  confirmed with `confirm` = (M, N): M matches in the last N frames; a track is dropped after more than max_misses consecutive
  misses, or when it is still tentative at age N.  A report that no live track holds in its gate starts a tentative track (when
  power / mean >= birth_ratio); a report inside the gate of a track that did not take it starts nothing, which suppresses
  duplicates beside a real track at the price of a late birth for a close neighbour.  An overflowing report list or a full table is
  an error, sticky in the table: TrackOverflowError, never a truncated answer.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _ffi, slot as _slot
from ._ffi import SarxError, check
from .slot import GmtiReport, encode as encode_slot   # noqa: F401

HEADER_BYTES = C.sizeof(_ffi.TrackHeader)
HEADER_DTYPE = np.dtype([("n_live", "<u4"), ("n_confirmed", "<u4"), ("next_id", "<i4"), ("frames_done", "<u4"), ("births_total", "<u4"),
                         ("drops_total", "<u4"), ("error", "<u4"), ("error_frame", "<i4"), ("max_tracks", "<u4"), ("reserved", "<u4", (7,))])
SLOT_DTYPE = np.dtype([("p_i", "<f8"), ("p_j", "<f8"), ("v_i", "<f8"), ("v_j", "<f8"), ("sum_re", "<f8"), ("sum_im", "<f8"),
                       ("sum_power", "<f8"), ("max_ratio", "<f8"), ("id", "<i4"), ("status", "<u4"), ("hits", "<u4"), ("misses", "<u4"),
                       ("age", "<u4"), ("hist", "<u4"), ("last_frame", "<i4"), ("last_report", "<i4")])
TRACK_DTYPE = np.dtype([("id", "<i4"), ("slot", "<i4"), ("confirmed", "?"), ("i", "<f8"), ("j", "<f8"), ("vel_i", "<f8"), ("vel_j", "<f8"),
                        ("hits", "<u4"), ("misses", "<u4"), ("age", "<u4"), ("last_frame", "<i4"), ("last_report", "<i4"),
                        ("interf", "<c16"), ("sum_power", "<f8"), ("max_ratio", "<f8"), ("range_rate_mps", "<f8"),
                        ("v_los_ati_mps", "<f8"), ("v_los_unwrapped_mps", "<f8")])
assert HEADER_DTYPE.itemsize == HEADER_BYTES == 64 and SLOT_DTYPE.itemsize == C.sizeof(_ffi.TrackSlot) == 96
_ERRORS = {_ffi.TRACK_ERR_SLOT_OVERFLOW: "a frame's report list overflowed", _ffi.TRACK_ERR_TABLE_OVERFLOW: "more births than free track slots"}


class TrackOverflowError(SarxError):
    """The tracker stopped at `frame`: a report list overflowed (kind "slot") or the table was full (kind "table")."""

    def __init__(self, error, frame):
        super().__init__(-1, f"GMTI tracker: {_ERRORS.get(int(error), 'error %d' % error)} at frame {frame}")
        self.kind = "slot" if int(error) == _ffi.TRACK_ERR_SLOT_OVERFLOW else "table"
        self.frame = int(frame)


@dataclass
class TrackParams:
    """gate (azimuth, range) half-widths in pixels; alpha, beta: position and velocity gains; confirm = (M, N); max_misses:
    consecutive misses a track survives; birth_ratio: power / mean a report needs to start a track (0 = none); max_tracks: table
    capacity; max_detections: capacity of the report lists (the detector's)."""
    gate: Tuple[float, float] = (4.0, 4.0)
    alpha: float = 0.5
    beta: float = 0.25
    confirm: Tuple[int, int] = (3, 5)
    max_misses: int = 3
    birth_ratio: float = 0.0
    max_tracks: int = 1024
    max_detections: int = 4096

    def check(self):
        try:
            ga, gr = (float(x) for x in self.gate)
            m, n = (int(x) for x in self.confirm)
        except (TypeError, ValueError):
            raise ValueError("gate must be (gate_az, gate_rg) and confirm (M, N)") from None
        if not (ga > 0 and gr > 0 and math.isfinite(ga) and math.isfinite(gr)):
            raise ValueError("gates must be finite and > 0")
        if not 0.0 < float(self.alpha) <= 1.0:
            raise ValueError("alpha must lie in (0, 1]")
        if not 0.0 <= float(self.beta) <= 2.0:
            raise ValueError("beta must lie in [0, 2]")
        if not 1 <= m <= n <= 32:
            raise ValueError("confirm = (M, N) needs 1 <= M <= N <= 32")
        if int(self.max_misses) < 0:
            raise ValueError("max_misses must be >= 0")
        if not (float(self.birth_ratio) >= 0.0 and math.isfinite(float(self.birth_ratio))):
            raise ValueError("birth_ratio must be finite and >= 0")
        if not 1 <= int(self.max_tracks) <= _ffi.TRACK_MAX_TRACKS:
            raise ValueError(f"max_tracks must be 1 .. {_ffi.TRACK_MAX_TRACKS}")
        if not 1 <= int(self.max_detections) <= _ffi.TRACK_MAX_DETECTIONS:
            raise ValueError(f"max_detections must be 1 .. {_ffi.TRACK_MAX_DETECTIONS}")
        return ga, gr, m, n

    def c_params(self):
        ga, gr, m, n = self.check()
        return _ffi.TrackParams(ga, gr, float(self.alpha), float(self.beta), float(self.birth_ratio), m, n, int(self.max_misses),
                                int(self.max_tracks), int(self.max_detections), 0)

    def slot_bytes(self):
        return _slot.slot_bytes(self.max_detections)


def table_bytes(cp):
    n = C.c_size_t()
    check(_ffi.load().sarx_track_table_bytes(C.byref(cp), C.byref(n)))
    return n.value


def workspace_bytes(cp):
    n = C.c_size_t()
    check(_ffi.load().sarx_track_workspace_bytes(C.byref(cp), C.byref(n)))
    return n.value


def enqueue_init(ctx, cp, table_ptr):
    check(ctx.lib.sarx_track_init_dev(ctx.h, C.byref(cp), table_ptr), ctx.h)


def enqueue_step(ctx, cp, slot_ptr, frame, table_ptr, assoc_ptr, workspace_ptr):
    """One step's two launches on the ctx's current lane; only enqueues."""
    check(ctx.lib.sarx_track_step_dev(ctx.h, C.byref(cp), slot_ptr, int(frame), table_ptr, assoc_ptr, workspace_ptr), ctx.h)


def enqueue_run(ctx, cp, stack_ptr, stride, n_frames, table_ptr, assoc_ptr, workspace_ptr):
    """Steps 0 .. n_frames - 1 over slots `stride` bytes apart; only enqueues."""
    check(ctx.lib.sarx_track_run_dev(ctx.h, C.byref(cp), stack_ptr, int(stride), int(n_frames), table_ptr, assoc_ptr, workspace_ptr), ctx.h)


class TrackResult:
    """`tracks`: the live table decoded (TRACK_DTYPE, rising slot index; the speeds are NaN without their scale); `header`;
    `assoc` [n_frames x max_detections] int32 (track id per report, -1 = none); `paths`: id -> dict(frames, reports, i, j) rebuilt
    from assoc, dropped tracks included; `raw`: the table's bytes."""

    def __init__(self, raw, assoc, frames_ij, frame_dt_s=None, dr_m=None, v_ambiguity_mps=None):
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self.raw, self.assoc = raw, np.asarray(assoc, np.int32)
        self.header = raw[:HEADER_BYTES].view(HEADER_DTYPE)[0]
        if int(self.header["error"]) != _ffi.TRACK_OK:
            raise TrackOverflowError(self.header["error"], self.header["error_frame"])
        slots = raw[HEADER_BYTES:].view(SLOT_DTYPE)
        live = np.flatnonzero(slots["status"] != _ffi.TRACK_FREE)
        s = slots[live]
        t = np.zeros(len(live), TRACK_DTYPE)
        t["slot"], t["confirmed"] = live, s["status"] == _ffi.TRACK_CONFIRMED
        for a, b in (("id", "id"), ("i", "p_i"), ("j", "p_j"), ("vel_i", "v_i"), ("vel_j", "v_j"), ("hits", "hits"), ("misses", "misses"),
                     ("age", "age"), ("last_frame", "last_frame"), ("last_report", "last_report"), ("sum_power", "sum_power"),
                     ("max_ratio", "max_ratio")):
            t[a] = s[b]
        t["interf"] = s["sum_re"] + 1j * s["sum_im"]
        nan = np.full(len(live), np.nan)
        t["range_rate_mps"] = t["vel_j"] * dr_m / frame_dt_s if dr_m is not None and frame_dt_s is not None else nan
        # GmtiReport.v_los_mps's convention: v_los = -lambda angle(interf) / (4 pi lag) = -v_amb angle / pi, receding positive
        t["v_los_ati_mps"] = -v_ambiguity_mps * np.angle(t["interf"]) / math.pi if v_ambiguity_mps is not None else nan
        t["v_los_unwrapped_mps"] = unwrap_speed(t["v_los_ati_mps"], t["range_rate_mps"], v_ambiguity_mps) if v_ambiguity_mps is not None else nan
        self.tracks = t
        self.frame_dt_s, self.dr_m, self.v_ambiguity_mps = frame_dt_s, dr_m, v_ambiguity_mps
        self.n_live, self.n_confirmed = int(self.header["n_live"]), int(self.header["n_confirmed"])
        self.paths = {}
        for f, ij in enumerate(frames_ij):
            row = self.assoc[f, :len(ij)]
            for r in np.flatnonzero(row >= 0):
                p = self.paths.setdefault(int(row[r]), dict(frames=[], reports=[], i=[], j=[]))
                p["frames"].append(f)
                p["reports"].append(int(r))
                p["i"].append(int(ij[r][0]))
                p["j"].append(int(ij[r][1]))

    def __repr__(self):
        return f"TrackResult({self.n_live} live, {self.n_confirmed} confirmed, {len(self.paths)} ids over {len(self.assoc)} frames)"


def unwrap_speed(v_ati, range_rate, v_amb):
    """The branch of the ATI speed (known modulo 2 v_amb) nearest to the coarse, unambiguous range rate."""
    return v_ati + 2.0 * v_amb * np.round((range_rate - v_ati) / (2.0 * v_amb))


def _slot_ij(raw, max_detections):
    rep = _slot.reports(raw, min(_slot.header(raw)[0], max_detections))
    return np.stack([rep["i"], rep["j"]], axis=1)


class GmtiTracker:
    """A track table on the device.  step(slot) enqueues one frame - a device slot (anything with .ptr, left alone until result())
    or host data (GmtiReport, report array, slot bytes; uploaded) - and never waits; result() downloads table and assoc."""

    def __init__(self, ctx, params, max_frames=256):
        self.ctx, self.params, self.max_frames = ctx, params, int(max_frames)
        self.cp = params.c_params()
        self.table = ctx.alloc(table_bytes(self.cp))
        self.ws = ctx.alloc(workspace_bytes(self.cp))
        self.d_assoc = ctx.alloc(self.max_frames * params.max_detections * 4)
        self._slots = []                     # per frame: host bytes, or the device buffer the caller keeps
        self._own = []
        enqueue_init(ctx, self.cp, self.table.ptr)

    def step(self, slot):
        f = len(self._slots)
        if f >= self.max_frames:
            raise ValueError(f"more than max_frames={self.max_frames} steps")
        _, stack, on_device = _slot.stage(slot, max_detections=self.params.max_detections, single=True)
        if on_device:
            ptr = slot.ptr
        else:
            self._own.append(self.ctx.to_device(stack[0]))
            ptr = self._own[-1].ptr
        self._slots.append(slot if on_device else stack[0])
        enqueue_step(self.ctx, self.cp, ptr, f, self.table.ptr, self.d_assoc.ptr + f * self.params.max_detections * 4, self.ws.ptr)
        return f

    def result(self, frame_dt_s=None, dr_m=None, v_ambiguity_mps=None):
        """Waits for the steps enqueued so far.  Raises TrackOverflowError if the table holds an error."""
        n, md = len(self._slots), self.params.max_detections
        raw = self.table.download(np.uint8, (self.table.nbytes,))
        assoc = self.d_assoc.download(np.int32, (self.max_frames, md))[:n].copy()
        ij = []
        for s in self._slots:
            if hasattr(s, "ptr"):
                s = _slot.fetch(self.ctx, s.ptr, md)
            ij.append(_slot_ij(s, md))
        return TrackResult(raw, assoc, ij, frame_dt_s, dr_m, v_ambiguity_mps)

    def close(self):
        for b in (self.table, self.ws, self.d_assoc, *self._own):
            b.release()
        self._own = []


def gmti_track(reports, params=None, *, frame_dt_s, dr_m=None, v_ambiguity_mps=None, ctx=None):
    """Track a sequence of frames: `reports` is a list of GmtiReport (gmti_detect, TwoChannelBatch.detections), of report arrays or
    of raw slots, in frame order, frame_dt_s apart.  All frames go up in one stack and the whole run is enqueued at once.

    dr_m: range pixel spacing, for range_rate_mps = vel_j dr / frame_dt; v_ambiguity_mps: lambda / (4 lag) (taken from the first
    GmtiReport when not given), for v_los_ati_mps from each track's summed interferogram and v_los_unwrapped_mps = v_ati +
    2 v_amb round((range_rate - v_ati) / (2 v_amb)).  Returns a TrackResult; raises TrackOverflowError."""
    from .engine import default_context
    params = params or TrackParams()
    cp = params.c_params()
    if not frame_dt_s > 0:
        raise ValueError("frame_dt_s must be > 0")
    reports = list(reports)
    if v_ambiguity_mps is None:
        v_ambiguity_mps = next((r.v_ambiguity_mps for r in reports if isinstance(r, GmtiReport)), None)
    md, stack, on_device = _slot.stage(reports, max_detections=params.max_detections)
    if on_device:
        raise TypeError("gmti_track takes host data; device slots go through GmtiTracker.step")
    n = len(stack)
    ctx = ctx or default_context()
    bufs = [ctx.to_device(stack if n else np.zeros((1, stack.shape[1]), np.uint8)), ctx.alloc(table_bytes(cp)), ctx.alloc(workspace_bytes(cp)),
            ctx.alloc(max(n, 1) * md * 4)]
    try:
        d_stack, table, ws, d_assoc = bufs
        enqueue_init(ctx, cp, table.ptr)
        enqueue_run(ctx, cp, d_stack.ptr, stack.shape[1], n, table.ptr, d_assoc.ptr, ws.ptr)
        raw = table.download(np.uint8, (table.nbytes,))
        assoc = d_assoc.download(np.int32, (max(n, 1), md))[:n]
    finally:
        for b in bufs:
            b.release()
    return TrackResult(raw, assoc, [_slot_ij(stack[f], md) for f in range(n)], frame_dt_s, dr_m, v_ambiguity_mps)
