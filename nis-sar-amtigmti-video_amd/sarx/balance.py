"""Two-channel balance on the GPU: a complex weight for channel 2 per image block, interpolated per pixel, and the coherence of
the two channels per block (include/sarx_balance.h, csrc/balance.hip).

Semantics (the kernels implement them; the host sizes the buffers and decodes the table):
  Blocks of block = (azimuth, range) pixels, ragged at the far edges.  Per block, over the pixels whose power in both channels is
  at most the clip level: S12 = sum slc1 conj(slc2), S11 = sum |slc1|^2, S22 = sum |slc2|^2 in fp64.  mode "ls": w = S12 / S22 (the
  least-squares fit of slc1 by w slc2), "phase": w = S12 / |S12|; coherence |S12| / sqrt(S11 S22).  Blocks with fewer than
  min_count kept pixels, no signal or a coherence below min_coherence take the global weight (the same formulas on the sums over
  the valid blocks).  interp "nearest": every pixel takes its block's weight, "bilinear": the weights are interpolated between the
  block centres, constant outside the outermost ones.  slc2 <- w slc2; everything downstream then runs with cal_phase = 0.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from ._ffi import SarxError, check

HEADER_BYTES = C.sizeof(_ffi.BalanceHeader)
HEADER_DTYPE = np.dtype([("nb_az", "<u4"), ("nb_rg", "<u4"), ("n_valid", "<u4"), ("reserved", "<u4"), ("w_re", "<f8"), ("w_im", "<f8"),
                         ("coherence", "<f8"), ("s11", "<f8"), ("s22", "<f8"), ("n", "<u8")])
RECORD_DTYPE = np.dtype([("s12_re", "<f8"), ("s12_im", "<f8"), ("s11", "<f8"), ("s22", "<f8"), ("w_re", "<f8"), ("w_im", "<f8"),
                         ("coherence", "<f4"), ("n", "<u4"), ("valid", "<u4"), ("reserved", "<u4")])
assert HEADER_DTYPE.itemsize == HEADER_BYTES == 64 and RECORD_DTYPE.itemsize == C.sizeof(_ffi.BalanceRecord) == 64

_MODES = {"ls": _ffi.BALANCE_LS, "phase": _ffi.BALANCE_PHASE}
_INTERPS = {"nearest": _ffi.BALANCE_NEAREST, "bilinear": _ffi.BALANCE_BILINEAR}


@dataclass
class BalanceParams:
    """block (azimuth, range) in pixels; mode "ls" or "phase"; interp "bilinear" or "nearest"; clip_db: pixels more than this many
    dB over the mean power of channel 1 stay out of the sums (None = all pixels); min_count: kept pixels a block needs (None = a
    quarter of a full block, of the image where the block is larger); min_coherence: coherence a block needs."""
    block: Tuple[int, int] = (256, 256)
    mode: str = "ls"
    interp: str = "bilinear"
    clip_db: Optional[float] = None
    min_count: Optional[int] = None
    min_coherence: float = 0.0

    def check(self):
        """Everything that does not depend on the image size; returns (block_az, block_rg).  Raises ValueError."""
        try:
            ba, br = (int(x) for x in self.block)
        except (TypeError, ValueError):
            raise ValueError("block must be (block_az, block_rg)") from None
        lo, hi = _ffi.BALANCE_MIN_BLOCK, _ffi.BALANCE_MAX_BLOCK
        if not (lo <= ba <= hi and lo <= br <= hi):
            raise ValueError(f"block {ba} x {br}: each side must be {lo} .. {hi}")
        if self.mode not in _MODES:
            raise ValueError(f"mode {self.mode!r} is not 'ls' or 'phase'")
        if self.interp not in _INTERPS:
            raise ValueError(f"interp {self.interp!r} is not 'bilinear' or 'nearest'")
        if self.clip_db is not None and not math.isfinite(float(self.clip_db)):
            raise ValueError("clip_db must be finite (None = no clip)")
        if not (0.0 <= float(self.min_coherence) <= 1.0):
            raise ValueError("min_coherence must lie in 0 .. 1")
        if self.min_count is not None and int(self.min_count) < 1:
            raise ValueError("min_count must be >= 1")
        return ba, br

    def resolved(self, n_az, n_rg):
        """(block_az, block_rg, mode, interp, min_count) for an [n_az x n_rg] image; raises ValueError on bad settings."""
        ba, br = self.check()
        if n_az < 1 or n_rg < 1:
            raise ValueError(f"bad image size {n_az} x {n_rg}")
        nb = -(-n_az // ba) * -(-n_rg // br)
        if nb > _ffi.BALANCE_MAX_BLOCKS:
            raise ValueError(f"{nb} blocks exceed {_ffi.BALANCE_MAX_BLOCKS}: use larger blocks")
        mc = self.min_count
        if mc is None:
            mc = max(min(ba, n_az) * min(br, n_rg) // 4, 1)
        return ba, br, _MODES[self.mode], _INTERPS[self.interp], int(mc)

    def c_params(self, n_az, n_rg, clip_power=math.inf):
        ba, br, mode, interp, mc = self.resolved(n_az, n_rg)
        if not clip_power > 0.0:
            raise ValueError("clip_power must be > 0")
        return _ffi.BalanceParams(ba, br, mode, interp, min(mc, 2 ** 31 - 1), 0, float(clip_power), float(self.min_coherence))


def table_bytes(cp, n_az, n_rg):
    n = C.c_size_t()
    check(_ffi.load().sarx_balance_table_bytes(C.byref(cp), int(n_az), int(n_rg), C.byref(n)))
    return n.value


def workspace_bytes(cp, n_az, n_rg):
    n = C.c_size_t()
    check(_ffi.load().sarx_balance_workspace_bytes(C.byref(cp), int(n_az), int(n_rg), C.byref(n)))
    return n.value


def enqueue_estimate(ctx, d_slc1, d_slc2, n_az, n_rg, cp, table_ptr, workspace_ptr):
    """The estimate's two launches on the ctx's current lane (device pointers, [n_az x n_rg] row-major); only enqueues."""
    check(ctx.lib.sarx_balance_estimate_dev(ctx.h, d_slc1, d_slc2, int(n_az), int(n_rg), C.byref(cp), table_ptr, workspace_ptr), ctx.h)


def enqueue_apply(ctx, d_slc1, d_slc2, n_az, n_rg, cp, table_ptr, out_ptr, dpca_ptr=None):
    """slc2_out = w slc2 (out_ptr may be d_slc2), optionally |slc1 - slc2_out| into dpca_ptr; only enqueues."""
    check(ctx.lib.sarx_balance_apply_dev(ctx.h, d_slc1, d_slc2, int(n_az), int(n_rg), C.byref(cp), table_ptr, out_ptr, dpca_ptr), ctx.h)


class ChannelBalance:
    """Result of a balance: the block table decoded ([nb_az x nb_rg] arrays `weights` complex128, `coherence`, `valid`, `counts`,
    the block sums `s12`, `s11`, `s22`; `global_weight`, `global_coherence`, `n_valid`) and, from channel_balance, the balanced
    image `slc2` (same kind and layout as the input) and `dpca_mag` (or None)."""

    def __init__(self, raw, shape, block, interp, clip_power, slc2=None, dpca_mag=None):
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        hdr = raw[:HEADER_BYTES].view(HEADER_DTYPE)[0]
        self.nb_az, self.nb_rg, self.n_valid = int(hdr["nb_az"]), int(hdr["nb_rg"]), int(hdr["n_valid"])
        rec = raw[HEADER_BYTES:HEADER_BYTES + self.nb_az * self.nb_rg * 64].view(RECORD_DTYPE).reshape(self.nb_az, self.nb_rg)
        self.raw = raw
        self.shape, self.block, self.interp, self.clip_power = (int(shape[0]), int(shape[1])), (int(block[0]), int(block[1])), interp, clip_power
        self.weights = rec["w_re"] + 1j * rec["w_im"]
        self.coherence = rec["coherence"].astype(np.float64)
        self.valid = rec["valid"] != 0
        self.counts = rec["n"].astype(np.int64)
        self.s12 = rec["s12_re"] + 1j * rec["s12_im"]
        self.s11, self.s22 = rec["s11"].copy(), rec["s22"].copy()
        self.global_weight = complex(hdr["w_re"], hdr["w_im"])
        self.global_coherence = float(hdr["coherence"])
        self.slc2, self.dpca_mag = slc2, dpca_mag

    def _axis(self, idx, n, block, nb):
        idx = np.asarray(idx)
        if np.any((idx < 0) | (idx >= n)):
            raise IndexError("pixel outside the image")
        if self.interp == "nearest":
            b = idx // block
            return b, b, np.zeros(idx.shape)
        t = np.clip((idx + 0.5) / block - 0.5, 0.0, nb - 1)
        b0 = np.minimum(np.floor(t).astype(np.int64), max(nb - 2, 0))
        return b0, np.minimum(b0 + 1, nb - 1), t - b0

    def _at(self, table, i, j):
        a0, a1, fa = self._axis(i, self.shape[0], self.block[0], self.nb_az)
        r0, r1, fr = self._axis(j, self.shape[1], self.block[1], self.nb_rg)
        return (1 - fa) * ((1 - fr) * table[a0, r0] + fr * table[a0, r1]) + fa * ((1 - fr) * table[a1, r0] + fr * table[a1, r1])

    def coherence_at(self, i, j):
        """Block coherence at pixel (i = azimuth, j = range), carried to the pixel the way the weight is (interp)."""
        return self._at(self.coherence, i, j)

    def weight_at(self, i, j):
        return self._at(self.weights, i, j)

    def __repr__(self):
        return (f"ChannelBalance({self.nb_az} x {self.nb_rg} blocks, {self.n_valid} valid, global weight {self.global_weight:.4g}, "
                f"global coherence {self.global_coherence:.4g})")


def _clip_power(ctx, p1, p2, n_az, n_rg, clip_db):
    """10^(clip_db / 10) mean |slc1|^2: the mean from an estimate with the largest blocks and no clip; only the header comes back."""
    big = BalanceParams(block=(_ffi.BALANCE_MAX_BLOCK, _ffi.BALANCE_MAX_BLOCK), mode="ls", interp="nearest", min_count=1)
    cp = big.c_params(n_az, n_rg)
    table, ws = ctx.alloc(table_bytes(cp, n_az, n_rg)), ctx.alloc(workspace_bytes(cp, n_az, n_rg))
    try:
        enqueue_estimate(ctx, p1, p2, n_az, n_rg, cp, table.ptr, ws.ptr)
        hdr = table.download(np.uint8, (HEADER_BYTES,)).view(HEADER_DTYPE)[0]
    finally:
        table.release()
        ws.release()
    if int(hdr["n_valid"]) == 0 or int(hdr["n"]) == 0 or not hdr["s11"] > 0:
        raise SarxError(-1, "channel balance: no signal common to both channels, the clip level has no reference")
    return 10.0 ** (float(clip_db) / 10.0) * float(hdr["s11"]) / float(hdr["n"])


def balance_dev(ctx, p1, p2, n_az, n_rg, params, out_ptr, dpca_ptr=None):
    """Estimate + apply on device pointers (out_ptr may be p2), then the table's download.  Returns (raw table bytes, clip_power).
    Raises SarxError when no block is valid."""
    clip = math.inf if params.clip_db is None else _clip_power(ctx, p1, p2, n_az, n_rg, params.clip_db)
    cp = params.c_params(n_az, n_rg, clip)
    table, ws = ctx.alloc(table_bytes(cp, n_az, n_rg)), ctx.alloc(workspace_bytes(cp, n_az, n_rg))
    try:
        enqueue_estimate(ctx, p1, p2, n_az, n_rg, cp, table.ptr, ws.ptr)
        enqueue_apply(ctx, p1 if dpca_ptr else None, p2, n_az, n_rg, cp, table.ptr, out_ptr, dpca_ptr)
        raw = table.download(np.uint8, (table.nbytes,))
    finally:
        table.release()
        ws.release()
    if int(raw[8:12].view("<u4")[0]) == 0:
        raise SarxError(-1, "channel balance: no valid block (too few pixels kept, no signal, or coherence below min_coherence); "
                            "the image was multiplied by 1")
    return raw, clip


def _image(ctx, x, temps, shape):
    """(device pointer, n_az, n_rg, kind) of an image given as a host [N_rg x N_az] array, a DeviceArray ([N_az x N_rg] or its .T)
    or a DeviceBuffer with shape=(n_az, n_rg)."""
    from .engine import DeviceArray, DeviceBuffer
    if isinstance(x, DeviceArray):
        mem = x.shape[::-1] if x.transposed else x.shape
        return x.ptr, mem[0], mem[1], "array"
    if isinstance(x, DeviceBuffer):
        if shape is None:
            raise ValueError("a DeviceBuffer image needs shape=(n_az, n_rg)")
        if x.nbytes < int(shape[0]) * int(shape[1]) * 8:
            raise ValueError("device buffer smaller than the image")
        return x.ptr, int(shape[0]), int(shape[1]), "buffer"
    a = np.asarray(x)
    if a.ndim != 2 or not np.iscomplexobj(a):
        raise ValueError("host images are 2-D complex arrays [N_rg x N_az] like sar_focus_csa's result")
    b = ctx.to_device(np.ascontiguousarray(a.T, dtype=np.complex64))
    temps.append(b)
    return b.ptr, a.shape[1], a.shape[0], "host"


def channel_balance(slc1, slc2, params=None, *, dpca_mag=False, in_place=False, shape=None, ctx=None):
    """Balance channel 2 against channel 1 block by block.

    slc1, slc2 : host [N_rg x N_az] complex arrays (sar_focus_csa's views) or device images ([N_az x N_rg] DeviceArray, or
                 DeviceBuffer with shape=(n_az, n_rg)), both of the same kind
    dpca_mag   : also |slc1 - w slc2| as a plane of the input's kind
    in_place   : the balanced image overwrites slc2 (a device image, or a writable complex64 host array) and is returned as .slc2
    Returns a ChannelBalance; raises SarxError when no block is valid."""
    from .engine import DeviceArray, default_context
    params = params or BalanceParams()
    params.check()
    if isinstance(slc1, np.ndarray) or isinstance(slc2, np.ndarray) or not (hasattr(slc1, "ptr") and hasattr(slc2, "ptr")):
        a1, a2 = np.asarray(slc1), np.asarray(slc2)
        if a1.ndim != 2 or a1.shape != a2.shape:
            raise ValueError("slc1 and slc2 must be 2-D images of the same shape and kind")
        if not (np.iscomplexobj(a1) and np.iscomplexobj(a2)):
            raise ValueError("host images are complex arrays [N_rg x N_az] like sar_focus_csa's result")
        params.resolved(a1.shape[1], a1.shape[0])             # before anything is uploaded
        if in_place and not (isinstance(slc2, np.ndarray) and slc2.dtype == np.complex64 and slc2.flags.writeable):
            raise ValueError("in_place on host images needs a writable complex64 array")
    ctx = ctx or getattr(slc1, "ctx", None) or default_context()
    temps = []
    try:
        p1, n_az, n_rg, kind = _image(ctx, slc1, temps, shape)
        p2, n_az2, n_rg2, kind2 = _image(ctx, slc2, temps, shape)
        if (n_az, n_rg, kind) != (n_az2, n_rg2, kind2):
            raise ValueError("slc1 and slc2 must be images of the same shape and kind")
        params.resolved(n_az, n_rg)
        n = n_az * n_rg
        if kind == "host" or in_place:
            out_buf, out_ptr = None, p2                        # a host image's upload is ours to overwrite
        else:
            out_buf = ctx.alloc(n * 8)
            out_ptr = out_buf.ptr
        dm = ctx.alloc(n * 4) if dpca_mag else None
        try:
            raw, clip = balance_dev(ctx, p1, p2, n_az, n_rg, params, out_ptr, dm.ptr if dm is not None else None)
        except Exception:
            for b in (out_buf, dm):
                if b is not None:
                    b.release()
            raise
        if kind == "host":
            img = temps[1].download(np.complex64, (n_az, n_rg)).T
            if in_place:
                slc2[...] = img
                img = slc2
            plane = None
            if dm is not None:
                plane = dm.download(np.float32, (n_az, n_rg)).T
                dm.release()
        else:
            plane = dm
            if in_place:
                img = slc2
            elif kind == "array":
                img = DeviceArray(out_buf, (n_az, n_rg))
                if slc2.transposed:
                    img = DeviceArray(out_buf, (n_rg, n_az), transposed=True)
            else:
                img = out_buf
        return ChannelBalance(raw, (n_az, n_rg), params.block, params.interp, clip, img, plane)
    finally:
        for b in temps:
            b.release()
