"""Call-trace recorder of the back-projection wrappers (sarx/tdbp*.py) against a stub context: no device, no library.

Every wrapper is driven with a context whose ``lib`` records each ``sarx_*`` call and returns 0 and whose ``alloc`` / ``to_device``
hand out stub buffers.  ``record()`` renders, per case, every library call (scalars by value, parameter blocks as bytes, geometry
and hypotheses as the fp64 values behind the pointer, every other pointer as NULL / host input i / host / stub device buffer
+ offset), every alloc, upload, download and release in order, the result, and the release accounting.  ``record(fail=True)`` lets
every launch entry return -1.  tests/test_tdbp_host_calls.py compares both with tests/golden/tdbp_host_calls.json;
``python tests/_tdbp_host_recorder.py --write FILE`` writes that file, ``--time`` prints the median wrapper overhead."""
import ctypes as C
import gc
import json
import os
import sys
import time
import weakref

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "nis-sar-amtigmti-video_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from sarx import _ffi, slot as _slot, tdbp as _tdbp  # noqa: E402
from sarx.engine import DeviceArray, DeviceBuffer  # noqa: E402
from sarx.tdbp import batch_constants, tdbp_gpu  # noqa: E402
from sarx.tdbp_multi import TdbpMultiResult, tdbp_multi  # noqa: E402
from sarx.tdbp_pair import tdbp_pair  # noqa: E402
from sarx.tdbp_pair_search import tdbp_pair_search  # noqa: E402
from sarx.tdbp_search import tdbp_search  # noqa: E402

N_P, N_S, NX, NY, N_HYP, CHIP = 6, 32, 8, 4, 3, (6, 4)
WINDOW = 1 << 36                      # stub device buffer k lives at (k + 1) * WINDOW
CTX_HANDLE = 0xC0FFEE
FP64 = []                             # the distinct fp64 arrays the library was handed, in the order they were first seen

# argument kinds per entry point: h handle, s scalar, B parameter block, O written by the stub, P [n_pulses x 3], T [n_pulses],
# V [3], H [n_hyp x 3] (all fp64 behind the pointer), p any other pointer, R the array of raw pointers
SPEC = {
    "sarx_tdbp_plan_create": "hssssBO", "sarx_tdbp_plan_destroy": "h", "sarx_tdbp_last_window": "hOO",
    "sarx_tdbp_focus_dev": "hpPPTsVsp", "sarx_tdbp_focus_host": "hpPPTsVspp",
    "sarx_tdbp_search_set_chunks": "hs", "sarx_tdbp_search_dev": "hpPPTsHsspp", "sarx_tdbp_search_host": "hpPPTsHsspp",
    "sarx_tdbp_search_route": "hO",
    "sarx_tdbp_pair_check": "sB", "sarx_tdbp_pair_dev": "hppPPTsVsBpp", "sarx_tdbp_pair_host": "hppPPTsVsBpp", "sarx_tdbp_pair_route": "hO",
    "sarx_tdbp_multi_check": "sB", "sarx_tdbp_multi_dev": "hRPPTsVsBpp", "sarx_tdbp_multi_host": "hRPPTsVsBpp", "sarx_tdbp_multi_route": "hO",
    "sarx_tdbp_pair_search_check": "Bss", "sarx_tdbp_pair_search_dev": "hppPPTssBHppsBppp", "sarx_tdbp_pair_search_route": "hO",
    "sarx_tdbp_multi_resolve_check": "B", "sarx_tdbp_multi_resolve_dev": "hBpsspp",
    "sarx_memcpy_d2h": "hpps",
}
LAUNCHES = {n for n in SPEC if n.endswith(("_dev", "_host"))}


class StubBuffer(DeviceBuffer):
    """A DeviceBuffer (the wrappers test for the class) without a device: an address window, its bytes, and counters."""

    def __init__(self, ctx, nbytes, data=None, mine=False):
        self.ctx, self.nbytes, self.index, self.mine, self.releases = ctx, int(nbytes), len(ctx.buffers), mine, 0
        self.ptr = (self.index + 1) * WINDOW
        self.data = bytes(data) if data is not None else None
        ctx.buffers.append(self)

    def release(self):
        self.releases += 1
        self.ctx.log.append(f"release dev{self.index}")

    def __del__(self):
        pass

    def download(self, dtype, shape):
        self.ctx.log.append(f"download dev{self.index} {np.dtype(dtype).name} {tuple(int(s) for s in shape)}")
        out = np.zeros(shape, dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("download larger than buffer")
        return out


class StubLib:
    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):                  # like ctypes.CDLL: made on first use, then an attribute
        if not name.startswith("sarx_"):
            raise AttributeError(name)
        setattr(self, name, lambda *args: self._ctx.call(name, args))
        return getattr(self, name)

    def sarx_last_error(self, ctx=None):
        return b"injected failure"


class StubContext:
    """What the wrappers ask a Context for.  ``tile``: what the route queries answer; ``k_best``: what the pair search's launch
    leaves in the first word of each best record; ``fail``: every launch entry returns -1."""

    def __init__(self, fail=False, tile=0, k_best=()):
        self.lib, self.h, self._lane, self._plans = StubLib(self), CTX_HANDLE, 0, weakref.WeakSet()
        self.fail, self.tile, self.k_best = fail, tile, k_best
        self.buffers, self.log, self.host_inputs, self.n_plans = [], [], [], 0

    # what the wrappers call
    def alloc(self, nbytes):
        b = StubBuffer(self, nbytes)
        self.log.append(f"alloc {int(nbytes)} -> dev{b.index}")
        return b

    def to_device(self, arr):
        a = np.ascontiguousarray(arr)
        b = StubBuffer(self, a.nbytes, a.tobytes())
        self.log.append(f"to_device {a.dtype.name} {a.shape} {self.where(a.ctypes.data)} -> dev{b.index}")
        return b

    # what the cases call
    def device_input(self, nbytes, data=None):
        return StubBuffer(self, nbytes, data, mine=True)

    def host_input(self, arr):
        self.host_inputs.append(arr)
        return arr

    def where(self, p):
        if isinstance(p, C.c_void_p):
            p = p.value
        if p is None:
            return "NULL"
        for i, a in enumerate(self.host_inputs):
            if a.ctypes.data <= p < a.ctypes.data + max(a.nbytes, 1):
                return f"host input {i}" + (f"+{p - a.ctypes.data}" if p != a.ctypes.data else "")
        k, off = divmod(int(p), WINDOW)
        if 1 <= k <= len(self.buffers):
            return f"dev{k - 1}" + (f"+{off}" if off else "")
        return "host"

    @staticmethod
    def _f64(p, n):
        """The n fp64 values at p, by their place in FP64 (each distinct array is written out once)."""
        vals = [repr(float(x)) for x in (C.c_double * n).from_address(p)]
        if vals not in FP64:
            FP64.append(vals)
        return f"fp64[{FP64.index(vals)}]"

    def call(self, name, args):
        spec = SPEC[name]
        assert len(spec) == len(args), (name, len(args))
        out = []
        for i, (kind, a) in enumerate(zip(spec, args)):
            if kind == "h":
                out.append("ctx" if a == CTX_HANDLE else "plan" if isinstance(a, C.c_void_p) and a.value else repr(a))
            elif kind == "s":
                out.append(repr(a))
            elif kind == "B":
                out.append(bytes(a._obj).hex())
            elif kind == "O":
                obj = a._obj
                if isinstance(obj, C.c_void_p):
                    self.n_plans += 1
                    obj.value = 0x1000 * self.n_plans
                else:
                    obj.value = self.tile
                out.append("out")
            elif kind in "PTVH":
                n_hyp = args[i + 1] if name.startswith("sarx_tdbp_search") else N_HYP       # the search passes its count next
                out.append(self._f64(a, {"P": 3 * N_P, "T": N_P, "V": 3, "H": 3 * n_hyp}[kind]))
            elif kind == "R":
                out.append([self.where(x) for x in a])
            else:
                out.append(self.where(a))
        self.log.append([name] + out)
        if name == "sarx_memcpy_d2h":
            k, off = divmod(int(args[2]), WINDOW)
            buf = self.buffers[k - 1]
            data = (buf.data or bytes(buf.nbytes))[off:off + int(args[3])]
            assert len(data) == int(args[3]), "download past the end of a stub buffer"
            C.memmove(args[1], data, len(data))
        if name in LAUNCHES and self.fail:
            return -1
        if name == "sarx_tdbp_pair_search_dev" and self.k_best:
            best = self.buffers[int(args[15]) // WINDOW - 1]
            rec = np.zeros(best.nbytes // 80 * 20, "<i4")
            rec[::20][:len(self.k_best)] = self.k_best
            best.data = rec.tobytes()
        return 0


# ---------------------------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------------------------
K = batch_constants()
V, PRF = float(K["V_sat"]), float(K["PRF"])
D = V / PRF
POS = np.stack([np.arange(N_P) * D, np.full(N_P, -4000.0), np.full(N_P, 350000.0)], axis=1)
VEL = np.tile([V, 0.0, 0.0], (N_P, 1))
TP = np.arange(N_P) / PRF
VF = (1.5, -2.5, 0.0)
HYPS = np.array([[0.0, -3.0, 0.0], [0.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
OFFS = {2: (-D, D), 3: (-D, D, 3 * D), 4: (-D, D, 3 * D, 5 * D)}
T_START, SCENE = 2.5e-3, 120.0
REPORTS = np.zeros(2, _slot.REPORT_DTYPE)
REPORTS["i"], REPORTS["j"], REPORTS["power"] = (1, 2), (3, 5), (4.0, 9.0)


def _host_raw(ctx, c):
    return ctx.host_input((np.arange(N_P * N_S).reshape(N_P, N_S) + 1j * c).astype(np.complex64))


def _dev_raw(ctx, as_array=False, shape=(N_P, N_S), transposed=False):
    buf = ctx.device_input(N_P * N_S * 8)
    return DeviceArray(buf, shape, owner=False, transposed=transposed) if as_array else buf


def _raws(ctx, n, device):
    return [_dev_raw(ctx, as_array=c % 2 == 1) if device else _host_raw(ctx, c) for c in range(n)]


def _dev_slot(ctx, md=4):
    return ctx.device_input(_slot.slot_bytes(md), _slot.encode(REPORTS, md))


def _arr(a):
    if isinstance(a, np.ndarray):
        return f"ndarray {a.dtype.name} {a.shape}"
    if isinstance(a, DeviceArray):
        return f"DeviceArray {a.shape} {ctx_where(a)} owner={a.owner}"
    return repr(a)


def ctx_where(a):
    return a.ctx.where(a.ptr)


def _render(res):
    """What a caller sees of a result."""
    if res is None or isinstance(res, np.ndarray):
        return _arr(res)
    out = {"type": type(res).__name__}
    for name in ("route", "lag_s", "lags_s", "v_ambiguity", "wavelength", "n_rx"):
        if hasattr(res, name):
            out[name] = repr(getattr(res, name))
    for name in ("img1", "img2", "images", "records", "best", "chips", "vel_hyps"):
        if hasattr(res, name):
            out[name] = _arr(getattr(res, name))
    if hasattr(res, "imgs"):
        out["imgs"] = _arr(res.imgs) if isinstance(res.imgs, np.ndarray) else [_arr(a) for a in res.imgs]
        out["pair(1)"] = [_arr(res.pair(1).img1), _arr(res.pair(1).img2), repr(res.pair(1).lag_s)]
    if hasattr(res, "k_best"):
        for name in ("k_best", "x0", "peak_ix", "s4", "interf"):
            out[name] = repr(getattr(res, name).tolist())
        if res.chips is not None:
            out["chips nan"] = repr(np.isnan(res.chips).all(axis=(1, 2, 3, 4)).tolist())
    return out


def _run(fail, fn, **stub):
    """One case: fn(ctx) -> result (or a list of them).  The trace, the result or the exception's type, then release() and the plans'
    close, then the accounting: every buffer the wrappers allocated released exactly once, none of the caller's released."""
    from sarx._ffi import SarxError
    ctx = StubContext(fail=fail, **stub)
    saved = _ffi.load
    _ffi.load = lambda: ctx.lib                  # check() asks the library for the message of a failed call
    case = {}
    try:
        results = fn(ctx)
        results = results if isinstance(results, list) else [results]
        case["result"] = [_render(r) for r in results]
        ctx.log.append("release()")
        for r in results:
            if hasattr(r, "release"):
                r.release()
    except (ValueError, SarxError) as e:
        case["raises"] = "SarxError" if isinstance(e, SarxError) else type(e).__name__
    finally:
        _ffi.load = saved
        ctx.log.append("close plans")
        for key in [k for k, p in _tdbp._plans.items() if p.ctx is ctx]:
            _tdbp._plans.pop(key).close()
    case["trace"] = ctx.log
    case["released"] = {f"dev{b.index}": b.releases for b in ctx.buffers if not b.mine}
    case["caller's released"] = sum(b.releases for b in ctx.buffers if b.mine)
    return case


def _pair_args(raws):
    return (*raws, POS, VEL, OFFS[2], T_START, N_S, TP, SCENE, NX, NY)


def _multi_args(raws, n):
    return (raws, POS, VEL, OFFS[n], T_START, N_S, TP, SCENE, NX, NY)


def cases():
    """name -> (fn(ctx), stub settings)."""
    out = {}

    def add(name, fn, **stub):
        assert name not in out
        out[name] = (fn, stub)

    gpu = lambda ctx, raw, **kw: tdbp_gpu(raw, POS, VEL, T_START, N_S, VF, TP, SCENE, NX, NY, ctx=ctx, **kw)  # noqa: E731
    add("gpu host", lambda c: gpu(c, _host_raw(c, 0)))
    add("gpu dev", lambda c: gpu(c, _dev_raw(c)))
    add("gpu dev twice", lambda c: [gpu(c, _dev_raw(c)), gpu(c, _dev_raw(c))])
    add("gpu dev d_image", lambda c: gpu(c, _dev_raw(c), d_image=c.device_input(NX * NY * 16)))
    add("gpu host d_image", lambda c: gpu(c, _host_raw(c, 0), d_image=c.device_input(NX * NY * 16)))
    add("gpu bad geometry", lambda c: tdbp_gpu(_host_raw(c, 0), POS[:, :2], VEL, T_START, N_S, VF, TP, SCENE, NX, NY, ctx=c))
    add("gpu bad raw", lambda c: gpu(c, _host_raw(c, 0)[:, :-1]))

    search = lambda ctx, raw, hyps=HYPS, **kw: tdbp_search(raw, POS, VEL, T_START, N_S, hyps, TP, SCENE, NX, NY, ctx=ctx, **kw)  # noqa: E731
    for images in (False, True):
        add(f"search host images={images}", lambda c, i=images: search(c, _host_raw(c, 0), images=i), tile=int(images))
        add(f"search dev images={images}", lambda c, i=images: search(c, _dev_raw(c), images=i), tile=int(images))
    add("search dev again", lambda c: [search(c, _dev_raw(c), HYPS[:2], images=True), search(c, _dev_raw(c), images=True),
                                       search(c, _dev_raw(c), images=True, chunks=3), search(c, _dev_raw(c))])
    add("search bad hyps", lambda c: search(c, _host_raw(c, 0), HYPS[:, :2]))
    add("search bad geometry", lambda c: tdbp_search(_host_raw(c, 0), POS, VEL[:-1], T_START, N_S, HYPS, TP, SCENE, NX, NY, ctx=c))

    def pair(ctx, device, **kw):
        return tdbp_pair(*_pair_args(_raws(ctx, 2, device)), ctx=ctx, vel_focus=VF, **kw)

    add("pair host complex128", lambda c: pair(c, False))
    add("pair host complex64", lambda c: pair(c, False, dtype=np.complex64), tile=1)
    add("pair dev", lambda c: pair(c, True))
    add("pair dev complex64", lambda c: pair(c, True, dtype=np.complex64))
    add("pair dev device_output", lambda c: pair(c, True, device_output=True), tile=1)
    add("pair host no shift", lambda c: pair(c, False, pulse_shift=False))
    add("pair dev explicit shift", lambda c: pair(c, True, pulse_shift=((2, 0), 4), chunks=3, chirp_centre=0.0))
    add("pair host chunks", lambda c: pair(c, False, chunks=3))
    add("pair mixed", lambda c: tdbp_pair(*_pair_args([_host_raw(c, 0), _dev_raw(c)]), ctx=c))
    add("pair device_output host", lambda c: pair(c, False, device_output=True))
    add("pair device_output complex128", lambda c: pair(c, True, device_output=True, dtype=np.complex128))
    add("pair bad dtype", lambda c: pair(c, False, dtype=np.float32))
    add("pair transposed", lambda c: tdbp_pair(*_pair_args([_dev_raw(c), _dev_raw(c, True, (N_S, N_P), True)]), ctx=c))
    add("pair mis-shaped", lambda c: tdbp_pair(*_pair_args([_dev_raw(c, True, (N_P, N_S - 1)), _dev_raw(c)]), ctx=c))
    add("pair small buffer", lambda c: tdbp_pair(*_pair_args([c.device_input(N_P * N_S * 8 - 8), _dev_raw(c)]), ctx=c))
    add("pair bad host raw", lambda c: tdbp_pair(*_pair_args([_host_raw(c, 0), _host_raw(c, 1)[:-1]]), ctx=c))
    add("pair bad offsets", lambda c: tdbp_pair(*_raws(c, 2, False), POS, VEL, OFFS[3], T_START, N_S, TP, SCENE, NX, NY, ctx=c))
    add("pair bad geometry", lambda c: tdbp_pair(*_raws(c, 2, False), POS, VEL, OFFS[2], T_START, N_S, TP, SCENE, NX, NY, ctx=c, vel_focus=(0.0, 1.0)))

    def multi(ctx, n, device, **kw):
        return tdbp_multi(*_multi_args(_raws(ctx, n, device), n), ctx=ctx, vel_focus=VF, **kw)

    for n in (2, 3, 4):
        add(f"multi {n} host complex128", lambda c, n=n: multi(c, n, False))
        add(f"multi {n} host complex64", lambda c, n=n: multi(c, n, False, dtype=np.complex64, chunks=3), tile=1)
        add(f"multi {n} dev", lambda c, n=n: multi(c, n, True))
        add(f"multi {n} dev complex64", lambda c, n=n: multi(c, n, True, dtype=np.complex64))
        add(f"multi {n} dev device_output", lambda c, n=n: multi(c, n, True, device_output=True), tile=1)
        add(f"multi {n} explicit ranges", lambda c, n=n: multi(c, n, n == 3, pulse_ranges=((1, 0, 2, 1)[:n], 4), chirp_centre=0.0))
    add("multi not whole pulses", lambda c: tdbp_multi(_raws(c, 3, False), POS, VEL, (-D, D, 2.3 * D), T_START, N_S, TP, SCENE, NX, NY, ctx=c))
    add("multi raws and offsets differ", lambda c: tdbp_multi(_raws(c, 2, False), POS, VEL, OFFS[3], T_START, N_S, TP, SCENE, NX, NY, ctx=c))
    add("multi mixed", lambda c: tdbp_multi(*_multi_args([_host_raw(c, 0), _dev_raw(c), _host_raw(c, 2)], 3), ctx=c))
    add("multi device_output host", lambda c: multi(c, 3, False, device_output=True))
    add("multi device_output complex128", lambda c: multi(c, 3, True, device_output=True, dtype=np.complex128))
    add("multi five offsets", lambda c: tdbp_multi(_raws(c, 5, False), POS, VEL, (-D, D, 3 * D, 5 * D, 7 * D), T_START, N_S, TP, SCENE, NX, NY, ctx=c))
    add("multi ranges of another length", lambda c: multi(c, 3, False, pulse_ranges=((1, 0), 4)))
    add("multi bad geometry", lambda c: tdbp_multi(_raws(c, 2, False), POS, VEL, OFFS[2], T_START, N_S, TP[:-1], SCENE, NX, NY, ctx=c))

    def psearch(ctx, device, reports, **kw):
        return tdbp_pair_search(*_pair_args(_raws(ctx, 2, device)), reports, HYPS, chip=CHIP, ctx=ctx, **kw)

    add("pair_search host reports", lambda c: psearch(c, False, REPORTS))
    add("pair_search dev slot", lambda c: psearch(c, True, _dev_slot(c), max_detections=4), tile=1)
    add("pair_search host chips ch0", lambda c: psearch(c, False, REPORTS, chips=True, source="ch0", pulse_shift=False, chirp_centre=0.0))
    add("pair_search dev raw host reports chips", lambda c: psearch(c, True, REPORTS, chips=True))
    add("pair_search outside", lambda c: psearch(c, False, REPORTS, chips=True), k_best=(1, -1))
    add("pair_search slot without capacity", lambda c: psearch(c, True, _dev_slot(c)))
    add("pair_search bad source", lambda c: psearch(c, False, REPORTS, source="ch1"))
    add("pair_search bad hyps", lambda c: tdbp_pair_search(*_pair_args(_raws(c, 2, False)), REPORTS, HYPS[:, :2], chip=CHIP, ctx=c))
    add("pair_search bad geometry", lambda c: tdbp_pair_search(*_raws(c, 2, False), POS[:-1], VEL, OFFS[2], T_START, N_S, TP, SCENE, NX, NY,
                                                               REPORTS, HYPS, chip=CHIP, ctx=c))
    add("pair_search mis-shaped", lambda c: tdbp_pair_search(*_pair_args([_host_raw(c, 0), _dev_raw(c, True, (N_P - 1, N_S))]), REPORTS, HYPS,
                                                             chip=CHIP, ctx=c))
    add("pair_search overflowed slot", lambda c: psearch(c, True, c.device_input(_slot.slot_bytes(4), _overflowed(4)), max_detections=4))

    lags = {n: tuple((np.array(OFFS[n])[1:] - OFFS[n][0]) / (2 * V)) for n in OFFS}

    def host_stack(ctx, n):
        return TdbpMultiResult(np.zeros((n, NY, NX), np.complex128), lags[n], K["C"] / K["FC"], "exact", ctx)

    def dev_stack(ctx, n):
        buf = ctx.device_input(n * NY * NX * 8)
        imgs = [DeviceArray(buf, (NY, NX), offset=c * NY * NX * 8, owner=False) for c in range(n)]
        return TdbpMultiResult(imgs, lags[n], K["C"] / K["FC"], "tile", ctx, None)       # the caller keeps the buffer here

    add("resolve host stack host reports", lambda c: host_stack(c, 3).resolve(REPORTS, 30.0))
    add("resolve host stack dev slot", lambda c: host_stack(c, 4).resolve(_dev_slot(c), 30.0, half=2, max_detections=4))
    add("resolve dev stack host reports", lambda c: dev_stack(c, 2).resolve(REPORTS, 30.0, max_detections=5))
    add("resolve dev stack dev slot", lambda c: dev_stack(c, 3).resolve(_dev_slot(c), 30.0, max_detections=4))
    add("resolve slot without capacity", lambda c: dev_stack(c, 3).resolve(_dev_slot(c), 30.0))
    add("resolve overflowed slot", lambda c: host_stack(c, 3).resolve(c.device_input(_slot.slot_bytes(4), _overflowed(4)), 30.0, max_detections=4))
    return out


def _overflowed(md):
    raw = _slot.encode(REPORTS, md)
    raw[4:8].view("<u4")[0] = 1
    return raw


def record(fail=False, only=None):
    return {name: _run(fail, fn, **stub) for name, (fn, stub) in cases().items() if only is None or name in only}


def golden():
    """Every case, then every case that reached a launch entry again with that entry failing."""
    del FP64[:]
    ok = record(False)
    launching = {name for name, case in ok.items() if any(isinstance(t, list) and t[0] in LAUNCHES for t in case["trace"])}
    return {"fp64": list(FP64), "ok": ok, "launch fails": record(True, launching)}


def timings(calls=200):
    """Median seconds per call of each wrapper on the stub (host raw, one plan kept across the calls)."""
    ctx = StubContext()
    raws = _raws(ctx, 4, False)
    stack = TdbpMultiResult(np.zeros((3, NY, NX), np.complex128), (2e-4, 6e-4), 0.03, "exact", ctx)
    todo = {
        "tdbp_gpu": lambda: tdbp_gpu(raws[0], POS, VEL, T_START, N_S, VF, TP, SCENE, NX, NY, ctx=ctx),
        "tdbp_search": lambda: tdbp_search(raws[0], POS, VEL, T_START, N_S, HYPS, TP, SCENE, NX, NY, ctx=ctx),
        "tdbp_pair": lambda: tdbp_pair(*_pair_args(raws[:2]), ctx=ctx),
        "tdbp_multi": lambda: tdbp_multi(*_multi_args(raws[:3], 3), ctx=ctx),
        "tdbp_pair_search": lambda: tdbp_pair_search(*_pair_args(raws[:2]), REPORTS, HYPS, chip=CHIP, ctx=ctx),
        "resolve": lambda: stack.resolve(REPORTS, 30.0),
    }
    out = {}
    gc.disable()
    for name, fn in todo.items():
        t = []
        for _ in range(calls + 20):
            del ctx.log[:], ctx.buffers[:]
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        out[name] = float(np.median(t[20:]))
    gc.enable()
    for key in [k for k, p in _tdbp._plans.items() if p.ctx is ctx]:
        _tdbp._plans.pop(key).close()
    return out


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write"]:
        with open(sys.argv[2], "w") as f:
            json.dump(golden(), f, indent=0, separators=(",", ":"))
            f.write("\n")
    elif sys.argv[1:2] == ["--time"]:
        for name, t in timings().items():
            print(f"{name:18s} {t * 1e6:9.2f} us")
