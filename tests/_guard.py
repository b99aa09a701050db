"""Guard bands and poison for device buffers: what a kernel did OUTSIDE its output, and which bytes of it it never wrote.

A GuardedBuffer owns one sarx_malloc allocation laid out as [zone | payload | zone].  Zones (and, on request, the payload) are
filled with byte 0xFF through sarx_memset: NaN as fp32 and fp64, -1 as int32, so the same pattern is a canary for writes (a
changed zone byte) and poison for reads (a NaN that reaches a result came from outside an input's extent).  `.ptr` is the payload's
start, so every wrapper that takes "something with .ptr" (Context.*, CsaPlan.run_pass, focus_dev, set_ati, ...) accepts it.

Zone size is a condition, not a tuning knob (zone_bytes): at least two rows of the largest leading dimension of the case and at
least 64 KiB, rounded up to a multiple of 4096 bytes, so the payload keeps the alignment a bare allocation has.  An overrun shorter
than the zone stays inside memory the test owns: these tests OBSERVE overruns, they never cause a fault.  An overrun longer than
the zone cannot be made safe by any test: it leaves the allocation, and whether it is then seen, lands in a neighbour or faults is
the device's business.  Nothing here provokes one.

guarded_run is the protocol of tests/test_gpu_guard.py - run once with every output poisoned and once zeroed, compare - written
against this interface only, so tests/test_guard_helper.py can drive it on a CPU box with a fake context and wrong fake kernels.
The module reads no environment variable and touches no pytest setting."""
import ctypes as C

import numpy as np

POISON = 0xFF
MIN_ZONE = 64 << 10
PAGE = 4096


def zone_bytes(largest_ld_bytes=0):
    """The zone for a case whose largest leading dimension (bytes per row of the widest array any argument has) is given."""
    z = max(2 * int(largest_ld_bytes), MIN_ZONE)
    return (z + PAGE - 1) // PAGE * PAGE


class ZoneDamage:
    """Changed canary bytes on one side of a payload.  first / last are byte offsets RELATIVE TO THE PAYLOAD START: negative on
    the 'before' side, >= nbytes on the 'after' side (so first - nbytes is how far past the end the first stray byte lies)."""

    def __init__(self, side, first, last, count, nbytes):
        self.side, self.first, self.last, self.count, self.nbytes = side, int(first), int(last), int(count), int(nbytes)

    def __repr__(self):
        rel = f"{self.first - self.nbytes} .. {self.last - self.nbytes} past the end" if self.side == "after" else \
            f"{-self.first} .. {-self.last} before the start"
        return f"ZoneDamage({self.side}: {self.count} bytes, payload offsets {self.first} .. {self.last} = {rel})"


class GuardedBuffer:
    """[zone | payload | zone] in one sarx_malloc allocation.  offset= places the payload that many bytes past the aligned
    position (the bytes skipped belong to the leading zone and are canaries too)."""

    def __init__(self, ctx, nbytes, zone=None, offset=0):
        zone = zone_bytes() if zone is None else int(zone)
        if zone < MIN_ZONE or zone % PAGE:
            raise ValueError(f"zone of {zone} bytes: must be >= {MIN_ZONE} and a multiple of {PAGE} (zone_bytes)")
        if nbytes < 0 or offset < 0:
            raise ValueError("nbytes and offset must be >= 0")
        self.ctx, self.nbytes, self.zone, self.offset = ctx, int(nbytes), zone, int(offset)
        self._lead = zone + self.offset
        self._total = self._lead + self.nbytes + zone
        p = C.c_void_p()
        self._check(ctx.lib.sarx_malloc(ctx.h, self._total, C.byref(p)))
        self.base = p.value
        self.ptr = self.base + self._lead
        live = getattr(ctx, "_live", None)
        if live is not None:
            live[id(self)] = self.base                       # freed with the context like a DeviceBuffer
        self._memset(self.base, POISON, self._total)

    # -- plumbing --
    def _check(self, rc):
        if rc != 0:
            msg = self.ctx.lib.sarx_last_error(self.ctx.h) if hasattr(self.ctx.lib, "sarx_last_error") else b""
            raise RuntimeError(f"libsarx error {rc}: {msg.decode(errors='replace') if msg else ''}")

    def _memset(self, ptr, value, n):
        if n:
            self._check(self.ctx.lib.sarx_memset(self.ctx.h, ptr, int(value), int(n)))

    def _d2h(self, ptr, n):
        out = np.empty(int(n), np.uint8)
        if n:
            self._check(self.ctx.lib.sarx_memcpy_d2h(self.ctx.h, out.ctypes.data, ptr, int(n)))
        return out

    def release(self):
        if self.base is not None and self.ctx.h is not None:
            self.ctx.lib.sarx_free(self.ctx.h, self.base)
            live = getattr(self.ctx, "_live", None)
            if live is not None:
                live.pop(id(self), None)
        self.base = self.ptr = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # -- payload --
    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError("upload larger than the payload")
        if arr.nbytes:
            self._check(self.ctx.lib.sarx_memcpy_h2d(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype=np.uint8, shape=None):
        dtype = np.dtype(dtype)
        if shape is None:
            shape = (self.nbytes // dtype.itemsize,)
        n = int(np.prod(shape)) * dtype.itemsize
        if n > self.nbytes:
            raise ValueError("download larger than the payload")
        return self._d2h(self.ptr, n).view(dtype).reshape(shape)

    def poison(self):
        self._memset(self.ptr, POISON, self.nbytes)
        return self

    def zero(self):
        self._memset(self.ptr, 0, self.nbytes)
        return self

    def restore_zones(self):
        """Canaries again (after a reported damage, so that the next check reports only new damage)."""
        self._memset(self.base, POISON, self._lead)
        self._memset(self.ptr + self.nbytes, POISON, self.zone)

    # -- canaries --
    def check_zones(self):
        """Both zones downloaded and compared with the canary: [] when clean, else one ZoneDamage per damaged side."""
        out = []
        lead = self._d2h(self.base, self._lead)
        bad = np.flatnonzero(lead != POISON)
        if bad.size:
            out.append(ZoneDamage("before", bad[0] - self._lead, bad[-1] - self._lead, bad.size, self.nbytes))
        tail = self._d2h(self.ptr + self.nbytes, self.zone)
        bad = np.flatnonzero(tail != POISON)
        if bad.size:
            out.append(ZoneDamage("after", self.nbytes + bad[0], self.nbytes + bad[-1], bad.size, self.nbytes))
        return out


def guarded(ctx, arr, zone=None, offset=0):
    """A GuardedBuffer holding a host array."""
    arr = np.ascontiguousarray(arr)
    return GuardedBuffer(ctx, arr.nbytes, zone, offset).upload(arr)


class Finding:
    """One thing guarded_run saw that the header does not allow.
    kind: 'zone' (side, first, last, count as ZoneDamage), 'unwritten' (a promised byte that differs between the poisoned and the
    zeroed run: not written, or accumulated into; first / last / count in payload byte offsets), 'stray' (a byte the header says is
    left alone that is no longer 0xFF in the poisoned run), 'nonfinite' (NaN / Inf in a promised element; first = byte offset of the
    first such element), 'input' (a const input that downloads differently from what was uploaded)."""

    def __init__(self, kind, buffer, run, first, last, count, side=None):
        self.kind, self.buffer, self.run, self.side = kind, buffer, run, side
        self.first, self.last, self.count = int(first), int(last), int(count)

    def __repr__(self):
        s = f" {self.side}" if self.side else ""
        return f"{self.kind}{s} in '{self.buffer}' ({self.run} run): {self.count} bytes, payload offsets {self.first} .. {self.last}"


def _span(kind, name, run, mask):
    bad = np.flatnonzero(mask)
    return [Finding(kind, name, run, bad[0], bad[-1], bad.size)] if bad.size else []


def guarded_run(call, inputs, outputs, promised=None, dtypes=None, sync=None):
    """The protocol of one case.
    call()    : enqueues the entry point under test (may return something; the two runs' return values are handed back)
    inputs    : {name: (GuardedBuffer, host array)} - uploaded before each run, compared bit for bit afterwards
    outputs   : {name: GuardedBuffer}
    promised  : {name: n bytes (a prefix), a boolean byte mask, None (scratch: content not defined), {"promised": .., "scratch": ..}
                (two byte masks: content promised / content not defined), or f(poisoned-run bytes) -> one of those}; default: every
                byte.  Bytes that are neither promised nor scratch must still be 0xFF after the poisoned run.
    dtypes    : {name: np.float32 / np.float64} - promised elements of that type must be finite (complex = pairs of these)
    sync()    : waits for the device (the downloads of libsarx block on every lane, so None is fine there)
    Returns (findings, results) with results[run][name] = payload bytes and results[run]['return'] = call()'s value."""
    promised, dtypes = promised or {}, dtypes or {}
    findings, results = [], {}
    for run in ("poisoned", "zeroed"):
        for buf, host in inputs.values():
            buf.upload(host)
        for buf in outputs.values():
            buf.poison() if run == "poisoned" else buf.zero()
        ret = call()
        if sync is not None:
            sync()
        results[run] = {"return": ret}
        for name, buf in list(outputs.items()) + [(k, v[0]) for k, v in inputs.items()]:
            for d in buf.check_zones():
                findings.append(Finding("zone", name, run, d.first, d.last, d.count, d.side))
                buf.restore_zones()
        for name, (buf, host) in inputs.items():
            host = np.ascontiguousarray(host)
            got = buf.download(np.uint8, (host.nbytes,))
            findings += _span("input", name, run, got != host.view(np.uint8).reshape(-1))
        for name, buf in outputs.items():
            results[run][name] = buf.download(np.uint8)
    for name, buf in outputs.items():
        p, z = results["poisoned"][name], results["zeroed"][name]
        want = promised.get(name, buf.nbytes)
        if callable(want):
            want = want(p)
        scratch = None
        if isinstance(want, dict):
            want, scratch = want["promised"], want.get("scratch")
        if want is None:                                     # scratch as a whole: the header promises no content, only the extent
            continue
        if isinstance(want, (int, np.integer)):
            mask = np.zeros(buf.nbytes, bool)
            mask[:int(want)] = True
        else:
            mask = np.asarray(want, bool)
        free = ~mask if scratch is None else ~mask & ~np.asarray(scratch, bool)
        findings += _span("unwritten", name, "poisoned vs zeroed", mask & (p != z))
        findings += _span("stray", name, "poisoned", free & (p != POISON))
        dt = dtypes.get(name)
        if dt is not None:
            item = np.dtype(dt).itemsize
            n = buf.nbytes // item
            whole = mask[:n * item].reshape(n, item).all(axis=1)
            for run, data in (("poisoned", p), ("zeroed", z)):
                bad = whole & ~np.isfinite(data[:n * item].view(dt))
                idx = np.flatnonzero(bad)
                if idx.size:
                    findings.append(Finding("nonfinite", name, run, idx[0] * item, idx[-1] * item + item - 1, idx.size * item))
    return findings, results
