"""Sliding-window coherence on the GPU through the C ABI (include/sarx_coherence.h) against the NumPy restatement of its semantics
(tests/_coherence_numpy.py, direct fp64 sums).

Bars.  coh and igram: 5e-7 absolute, no pixel left out.  Both are at most 1 in modulus and are rounded once to fp32 (<= 6e-8); the
kernel's fp64 sums are running sums restarted at every tile, which differ from the direct ones by at most (additions) x 2^-53 x (the
largest power the running sum has held / the sum): <= 1e-7 with a point target 80 dB over unit speckle, the stated limit of dynamic
range of these tests.  5e-7 is 4 fp32 ulps of 1.0.  Mask and counts: exactly the restatement's; every case first asserts on the
restatement that no pixel's coh lies within 5e-7 of the threshold and no window sum within 1e-12 (relative) of power_floor N, so
the last bits of a sum cannot move a pixel across the rule (the seeds were chosen on the CPU so that this holds).  sum_coh: 1e-12
relative to the fp64 sum of the coh plane the call emitted, over the restatement's tested pixels (fp64 sums of the same fp32 values
in another order; the emitted fp32 coh may differ from the restatement's by one rounding, which the first bar allows), and within
5e-7 per tested pixel of the restatement's own sum."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coherence_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 5e-7
THR, FLOOR = 0.5, 0.5
WINDOWS = [(0, 0), (1, 1), (2, 3), (4, 4), (16, 16), (16, 0), (0, 16)]
KINDS = ["rho0", "rho05", "rho099", "phase", "zeros", "patch", "point"]
TILE = (64, 224)                                    # the kernel's tile: one row and one column past it below

# (shape, window, kind, payload offset in bytes)
CASES = [(s, (16, 16), k, 0) for s in ((1, 1), (1, 130), (130, 1), (5, 7)) for k in ("rho05", "point")]
CASES += [(s, w, k, 0) for s in ((96, 80), (257, 130)) for w in WINDOWS for k in KINDS]
CASES += [((33, 65), (2, 3), "rho05", 0), ((33, 65), (16, 16), "point", 8),
          ((TILE[0] + 1, TILE[1] + 1), (2, 3), "rho05", 0), ((TILE[0] + 1, TILE[1] + 1), (16, 16), "point", 8),
          ((TILE[0] + 1, TILE[1] + 1), (0, 0), "patch", 8), ((64, 64), (4, 4), "rho0", 0), ((64, 64), (1, 1), "point", 8),
          ((96, 80), (4, 4), "rho05", 8), ((257, 129), (2, 3), "point", 8), ((257, 129), (16, 0), "patch", 0),
          ((1000, 777), (4, 4), "point", 0), ((1000, 777), (16, 16), "patch", 8), ((1000, 777), (0, 16), "rho05", 8),
          ((1000, 777), (0, 0), "point", 0)]


# cases whose first seed leaves a pixel within 5e-7 of the threshold on the restatement (found on the CPU): they take a later seed
SEED_BUMP = {((257, 130), (16, 16), "rho05"): 1, ((1000, 777), (0, 16), "rho05"): 3}


def _seed(shape, window, kind):
    return 1 + shape[0] * 7 + shape[1] * 13 + window[0] * 101 + window[1] * 211 + KINDS.index(kind) * 1009 + \
        100003 * SEED_BUMP.get((shape, window, kind), 0)


_REF = {}


def _reference(shape, window, kind):
    """(a, b, restatement) of a case, computed once and shared."""
    key = (shape, window, kind)
    if key not in _REF:
        a, b = ref.pair(shape, kind, _seed(shape, window, kind))
        r = ref.coherence(a, b, window, THR, FLOOR)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _REF[key] = (a, b, r)
    return _REF[key]


class Run:
    """Device buffers of one pair call; offsets place every payload `off` bytes past its allocation's start."""

    def __init__(self, ctx, a, b, off=0, igram=True, mask=True, summary=True):
        self.K = importlib.import_module("sarx.coherence")
        self.ctx, self.shape, self.off = ctx, a.shape, off
        n = a.size
        self.bufs = {"a": ctx.alloc(n * 8 + off), "b": ctx.alloc(n * 8 + off), "coh": ctx.alloc(n * 4 + off)}
        if igram:
            self.bufs["igram"] = ctx.alloc(n * 8 + off)
        if mask:
            self.bufs["mask"] = ctx.alloc(n + off)
        if summary:
            self.bufs["summary"] = ctx.alloc(64 + off)
        self.ws = None
        for k, x in (("a", a), ("b", b)):
            self._up(k, x)

    def ptr(self, k):
        return self.bufs[k].ptr + self.off if k in self.bufs else None

    def _up(self, k, arr):
        arr = np.ascontiguousarray(arr)
        self.ctx.lib.sarx_memcpy_h2d(self.ctx.h, self.ptr(k), arr.ctypes.data, arr.nbytes)

    def fill(self, value):
        for k in ("coh", "igram", "mask", "summary"):
            if k in self.bufs:
                assert self.ctx.lib.sarx_memset(self.ctx.h, self.bufs[k].ptr, value, self.bufs[k].nbytes) == 0

    def get(self, k, dtype, shape):
        out = np.empty(shape, dtype)
        assert self.ctx.lib.sarx_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr(k), out.nbytes) == 0
        return out

    def call(self, window, threshold=THR, floor=FLOOR, raw=False, **override):
        from sarx import _ffi
        cp = _ffi.CoherenceParams(window[0], window[1], 0, 0, threshold, floor)
        if self.ws is None and "summary" in self.bufs:
            self.ws = self.ctx.alloc(self.K.workspace_bytes(_ffi.CoherenceParams(0, 0, 0, 0, 0.0, 0.0), *self.shape))
        args = {k: self.ptr(k) for k in ("a", "b", "coh", "igram", "mask", "summary")}
        args["ws"] = self.ws.ptr if self.ws else None
        args.update(override)
        rc = self.ctx.lib.sarx_coherence_pair_dev(self.ctx.h, args["a"], args["b"], self.shape[0], self.shape[1], C.byref(cp), args["coh"],
                                                  args["igram"], args["mask"], args["summary"], args["ws"])
        if not raw:
            assert rc == 0, self.ctx.last_error()
        return rc

    def results(self):
        out = {"coh": self.get("coh", np.float32, self.shape)}
        if "igram" in self.bufs:
            out["igram"] = self.get("igram", np.complex64, self.shape)
        if "mask" in self.bufs:
            out["mask"] = self.get("mask", np.uint8, self.shape)
        if "summary" in self.bufs:
            out["summary"] = self.get("summary", np.uint8, (64,))
        return out

    def release(self):
        for b in list(self.bufs.values()) + ([self.ws] if self.ws else []):
            b.release()


def _ids(c):
    return f"{c[0][0]}x{c[0][1]}-w{c[1][0]}_{c[1][1]}-{c[2]}-off{c[3]}"


@pytest.mark.parametrize("shape,window,kind,off", CASES, ids=[_ids(c) for c in CASES])
def test_pair_against_the_restatement(shape, window, kind, off):
    import sarx
    K = importlib.import_module("sarx.coherence")
    ctx = sarx.default_context()
    a, b, r = _reference(shape, window, kind)
    assert ref.clear_of_the_rule(r, THR, FLOOR), "the seed of this case leaves a pixel on the rule's edge: choose another"
    run = Run(ctx, a, b, off)
    try:
        run.fill(0xFF)
        run.call(window)
        got = run.results()
        run.fill(0x00)
        run.call(window)
        again = run.results()
    finally:
        run.release()
    for k in got:                                                         # two runs, byte for byte (and every byte written)
        assert got[k].tobytes() == again[k].tobytes(), k
    e_coh = float(np.max(np.abs(got["coh"].astype(np.float64) - np.minimum(np.abs(r["g"]), 1.0))))
    e_ig = float(np.max(np.abs(got["igram"].astype(np.complex128) - r["g"])))
    sm = got["summary"].view(K.SUMMARY_DTYPE)[0]
    print(f"{_ids((shape, window, kind, off))}: coh err {e_coh:.2e}, igram err {e_ig:.2e}, tested {int(sm['n_tested'])}, "
          f"changed {int(sm['n_changed'])}")
    assert np.isfinite(got["coh"]).all() and got["coh"].max() <= 1.0 and got["coh"].min() >= 0.0
    assert e_coh <= BOUND and e_ig <= BOUND
    np.testing.assert_array_equal(got["mask"], r["mask"])
    assert int(sm["n_tested"]) == r["n_tested"] and int(sm["n_changed"]) == r["n_changed"]
    emitted = float(got["coh"][r["tested"]].astype(np.float64).sum())   # sum_coh is the sum of the EMITTED coh over the tested pixels
    assert abs(float(sm["sum_coh"]) - emitted) <= 1e-12 * max(emitted, 1e-300)
    assert abs(float(sm["sum_coh"]) - r["sum_coh"]) <= BOUND * max(r["n_tested"], 1)
    assert int(sm["n_az"]) == shape[0] and int(sm["n_rg"]) == shape[1] and not sm["reserved"].any()
    if kind == "zeros":
        assert not got["coh"].any() and not got["igram"].view(np.float32).any() and not got["mask"].any()


def test_optional_outputs_do_not_change_the_required_one():
    import sarx
    ctx = sarx.default_context()
    shape, window = (257, 130), (4, 4)
    a, b, r = _reference(shape, window, "point")
    full = Run(ctx, a, b)
    bare = Run(ctx, a, b, igram=False, mask=False, summary=False)
    part = Run(ctx, a, b, igram=False, mask=True, summary=False)
    try:
        for x in (full, bare, part):
            x.fill(0xFF)
            x.call(window)
        f, g, h = full.results(), bare.results(), part.results()
    finally:
        for x in (full, bare, part):
            x.release()
    assert f["coh"].tobytes() == g["coh"].tobytes() == h["coh"].tobytes()
    assert f["mask"].tobytes() == h["mask"].tobytes()


@pytest.mark.parametrize("lag", [1, 2])
def test_stack_equals_the_loop_of_pairs(lag):
    import sarx
    K = importlib.import_module("sarx.coherence")
    ctx = sarx.default_context()
    nf, shape, window = 5, (96, 80), (2, 3)
    n = shape[0] * shape[1]
    frames = np.stack([ref.pair(shape, "rho05", 50 + f)[f % 2] for f in range(nf)])
    frames[3] = (0.8 * frames[1] + 0.6 * frames[3]).astype(np.complex64)
    pairs = nf - lag
    cp = sarx.CoherenceParams(window=window, threshold=THR, power_floor=FLOOR).c_params()
    d = ctx.to_device(frames)
    bufs = {"coh": ctx.alloc(pairs * n * 4), "igram": ctx.alloc(pairs * n * 8), "mask": ctx.alloc(pairs * n), "summary": ctx.alloc(pairs * 64),
            "ws": ctx.alloc(K.workspace_bytes(cp, *shape))}
    try:
        K.enqueue_stack(ctx, d.ptr, nf, n * 8, lag, shape[0], shape[1], cp, bufs["coh"].ptr, n * 4, bufs["igram"].ptr, n * 8,
                        bufs["mask"].ptr, n, bufs["summary"].ptr, bufs["ws"].ptr)
        got = {"coh": np.array(bufs["coh"].download(np.float32, (pairs,) + shape)),
               "igram": np.array(bufs["igram"].download(np.complex64, (pairs,) + shape)),
               "mask": np.array(bufs["mask"].download(np.uint8, (pairs,) + shape)),
               "summary": np.array(bufs["summary"].download(np.uint8, (pairs, 64)))}
        for f in range(pairs):
            run = Run(ctx, frames[f], frames[f + lag])
            try:
                run.call(window)
                one = run.results()
            finally:
                run.release()
            for k in one:
                assert one[k].tobytes() == got[k][f].tobytes(), (k, f)
            r = ref.coherence(frames[f], frames[f + lag], window, THR, FLOOR)
            assert np.max(np.abs(got["coh"][f].astype(np.float64) - np.minimum(np.abs(r["g"]), 1.0))) <= BOUND
        # the Python form: one upload, one download per plane
        res = sarx.coherence_stack(frames, sarx.CoherenceParams(window=window, threshold=THR, power_floor=FLOOR), lag=lag, igram=True, mask=True)
        assert res.coh.tobytes() == got["coh"].tobytes() and res.igram.tobytes() == got["igram"].tobytes()
        assert res.mask.tobytes() == got["mask"].tobytes()
        sm = got["summary"].reshape(-1).view(K.SUMMARY_DTYPE)
        assert res.n_tested.tolist() == sm["n_tested"].tolist() and res.n_changed.tolist() == sm["n_changed"].tolist()
        only = sarx.coherence_stack(frames, sarx.CoherenceParams(window=window, threshold=THR, power_floor=FLOOR), lag=lag, maps=False)
        assert only.coh is None and only.summary.tobytes() == sm.tobytes()
    finally:
        d.release()
        for v in bufs.values():
            v.release()


def test_refusals_write_nothing():
    import sarx
    from sarx import _ffi
    ctx = sarx.default_context()
    shape = (96, 80)
    n = shape[0] * shape[1]
    a, b, _ = _reference(shape, (4, 4), "rho05")
    run = Run(ctx, a, b)
    try:
        run.fill(0xFF)
        nan = float("nan")
        assert run.call((17, 4), raw=True) == -1 and run.call((4, -1), raw=True) == -1
        assert run.call((4, 4), threshold=nan, raw=True) == -1 and run.call((4, 4), threshold=-0.5, raw=True) == -1
        assert run.call((4, 4), floor=nan, raw=True) == -1 and run.call((4, 4), floor=-1.0, raw=True) == -1
        assert run.call((4, 4), raw=True, a=run.ptr("a") + 4) == -1                        # misaligned
        assert run.call((4, 4), raw=True, igram=run.ptr("igram") + 4) == -1
        assert run.call((4, 4), raw=True, coh=run.ptr("coh") + 2) == -1
        assert run.call((4, 4), raw=True, coh=run.ptr("a")) == -1                          # aliasing: output on an input
        assert run.call((4, 4), raw=True, igram=run.ptr("b")) == -1
        assert run.call((4, 4), raw=True, coh=run.ptr("igram") + 8) == -1                  # two outputs overlap
        assert run.call((4, 4), raw=True, ws=None) == -1                                   # a summary without the workspace
        assert run.call((4, 4), raw=True, a=None) == -1 and run.call((4, 4), raw=True, coh=None) == -1
        cp = _ffi.CoherenceParams(4, 4, 0, 0, THR, FLOOR)
        lib = ctx.lib
        for nf, lag in ((1, 1), (2, 2), (2, 0), (2, 5)):                                   # lag >= n_frames (the two images as a stack of one)
            assert lib.sarx_coherence_stack_dev(ctx.h, run.ptr("a"), nf, n * 8, lag, shape[0], shape[1], C.byref(cp), run.ptr("coh"), n * 4,
                                                run.ptr("igram"), n * 8, run.ptr("mask"), n, run.ptr("summary"), run.ws.ptr) == -1
        assert lib.sarx_coherence_stack_dev(ctx.h, run.ptr("a"), 1, n * 8 - 8, 1, shape[0], shape[1], C.byref(cp), run.ptr("coh"), n * 4,
                                            None, 0, None, 0, None, None) == -1
        ctx.sync()
        for k, v in run.results().items():
            assert (v.view(np.uint8) == 0xFF).all(), k
        assert np.array_equal(run.get("a", np.complex64, shape), a) and np.array_equal(run.get("b", np.complex64, shape), b)
        run.call((4, 4))                                                                   # and the good call still runs
        assert np.isfinite(run.results()["coh"]).all()
    finally:
        run.release()


def test_python_interface():
    import sarx
    shape, window = (96, 80), (4, 4)
    a, b, (i0, j0, size) = ref.change_scene()
    r = ref.coherence(a, b, window, 0.5, 0.0)
    assert ref.clear_of_the_rule(r, 0.5, 0.0)
    p = sarx.CoherenceParams(window=window, threshold=0.5)
    res = sarx.coherence(a.T, b.T, p, igram=True, mask=True)             # host images are [N_rg x N_az] views
    assert res.coh.shape == shape[::-1] and res.coh.dtype == np.float32 and res.mask.dtype == np.uint8
    np.testing.assert_array_equal(res.mask.T, r["mask"])
    assert np.max(np.abs(res.coh.T.astype(np.float64) - np.minimum(np.abs(r["g"]), 1.0))) <= BOUND
    assert np.max(np.abs(res.igram.T.astype(np.complex128) - r["g"])) <= BOUND
    assert (res.n_tested, res.n_changed) == (r["n_tested"], r["n_changed"]) and abs(res.mean_coh - r["sum_coh"] / r["n_tested"]) < 1e-12
    assert (res.mask.T[i0 + 6:i0 + size - 6, j0 + 6:j0 + size - 6] == 2).all() and (res.mask.T[:i0 - 6] == 1).all()
    plain = sarx.coherence(a.T, b.T, sarx.CoherenceParams(window=window))
    assert plain.igram is None and plain.mask is None and plain.n_tested is None and plain.coh.tobytes() == res.coh.tobytes()
    ctx = sarx.default_context()
    da, db = sarx.DeviceArray(ctx.to_device(a), shape), sarx.DeviceArray(ctx.to_device(b), shape)
    dev = sarx.coherence(da, db, p, mask=True, device_output=True)
    try:
        assert np.array(dev.coh.download(np.float32, shape)).tobytes() == res.coh.T.tobytes()
        assert np.array(dev.mask.download(np.uint8, shape)).tobytes() == res.mask.T.tobytes() and dev.n_changed == res.n_changed
    finally:
        dev.release()
        da.release()
        db.release()


@pytest.mark.parametrize("with_balance", [False, True], ids=["plain", "balance"])
def test_focus_ati_dpca_with_coherence(with_balance):
    """256 x 256, the two-channel point-target scene: res["coherence"] is sarx.coherence of the images the products came from, bit
    for bit, and within the bound of the restatement on the downloaded images; every other key is what the call without
    coherence= returns."""
    import sarx
    from oracle import csa_oracle as orc
    (r1, r2), k = orc.point_scene(256, 256, seed=5, clutter_db=-25.0, two_channel=True)
    args = orc.focus_args(k)
    kw = dict(pulse_shift=False)
    if with_balance:
        kw["balance"] = sarx.BalanceParams(block=(64, 64))
    p = sarx.CoherenceParams(window=(2, 2), threshold=0.6, power_floor=0.0)
    base = sarx.focus_ati_dpca(r1, r2, *args, **kw)
    res = sarx.focus_ati_dpca(r1, r2, *args, coherence=p, **kw)
    new = {"coherence", "coherence_mask", "coherence_n_tested", "coherence_n_changed", "coherence_mean"}
    assert set(res) - set(base) == new and set(base) <= set(res)
    for key, v in base.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == res[key].tobytes() and v.shape == res[key].shape, key
        elif key == "balance":
            assert v.raw.tobytes() == res[key].raw.tobytes()
        else:
            assert v == res[key], key
    alone = sarx.coherence(res["slc1"], res["slc2"], p, mask=True)
    assert alone.coh.tobytes() == res["coherence"].tobytes() and alone.mask.tobytes() == res["coherence_mask"].tobytes()
    assert (alone.n_tested, alone.n_changed) == (res["coherence_n_tested"], res["coherence_n_changed"])
    assert alone.mean_coh == res["coherence_mean"]
    r = ref.coherence(np.ascontiguousarray(res["slc1"].T), np.ascontiguousarray(res["slc2"].T), (2, 2), 0.6, 0.0)
    err = float(np.max(np.abs(res["coherence"].T.astype(np.float64) - np.minimum(np.abs(r["g"]), 1.0))))
    print(f"focus_ati_dpca coherence err {err:.2e}, changed {res['coherence_n_changed']} of {res['coherence_n_tested']}")
    assert err <= BOUND
    # without a threshold: the map alone; and channel 2 is kept on the device for it even when it is not returned
    bare = sarx.focus_ati_dpca(r1, r2, *args, coherence=sarx.CoherenceParams(window=(2, 2)), return_slc2=False, **kw)
    assert bare["coherence"].tobytes() == res["coherence"].tobytes() and "coherence_mask" not in bare
    assert ("slc2" in bare) == ("slc2" in sarx.focus_ati_dpca(r1, r2, *args, return_slc2=False, **kw))
