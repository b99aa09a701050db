"""Focus-velocity search of the back-projection on the GPU (include/sarx_tdbp_search.h): the image stack against
oracle/tdbp_oracle.py per hypothesis (relative L2 < 1e-4, the bar of tests/test_gpu_tdbp.py) and against sarx.tdbp_gpu (< 2e-6, the
bar the two focus kernels hold against each other), the records against fp64 NumPy sums over the device's own stack, bit identity,
the device-resident input, recovery of the along-track velocity on the scene of tests/test_tdbp_search.py, and the refusals."""
import contextlib
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

from oracle import tdbp_oracle as tb
from oracle.csa_oracle import rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_search_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
KERNEL_TOL = 2e-6


def _args(sc, raw=None):
    return (sc["raw"].astype(np.complex64) if raw is None else raw, sc["pos"], sc["vel"], sc["t_start"], sc["num_samples"])


@contextlib.contextmanager
def _route(case):
    """The 160-pulse, 400 m, 40 x 40 scene meets the tile condition of the focus (5 u^4 / 128 d = 8.5e-10 m against 1e-9 m), so left
    alone it takes the tile kernel - in tdbp_gpu as in the search.  The exact kernel is checked on it all the same, through the
    switch the focus tests use (SARX_TDBP_TILE=0, read by the shared condition at every call); "coarse" takes it by geometry."""
    if case != "exact":
        yield
        return
    old = os.environ.get("SARX_TDBP_TILE")
    os.environ["SARX_TDBP_TILE"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["SARX_TDBP_TILE"]
        else:
            os.environ["SARX_TDBP_TILE"] = old


def _search(sc, hyps, nx, ny, raw=None, case="tile", **kw):
    import sarx
    with _route(case):
        return sarx.tdbp_search(*_args(sc, raw), hyps, sc["t_vec"], sc["swath"], nx, ny, consts=sc["k"], **kw)


def _hyps(sc):
    return np.array([np.zeros(3), sc["v_tgt"], sc["v_tgt"] + np.array([6.0, -0.2, 0.0])])


@pytest.fixture(scope="module")
def tile_case():
    """The scene of test_tile_expansion_equals_exact_kernel: ragged 90 x 70 tiles, 320 pulses in ten chunks of 32."""
    sc = tb.tdbp_scene(n_pulses=320, seed=21, k=tb.batch_constants(), speed=15.0, heading_deg=45.0, swath=90.0, n_targets=4)
    hyps = _hyps(sc)
    return sc, hyps, ref.stack_images(sc, hyps, 90, 70), _search(sc, hyps, 90, 70, images=True)


@pytest.fixture(scope="module")
def exact_case():
    sc = tb.tdbp_scene(n_pulses=160, seed=2, k=tb.scaled_constants(), swath=400.0)
    hyps = _hyps(sc)
    return sc, hyps, ref.stack_images(sc, hyps, 40, 40), _search(sc, hyps, 40, 40, images=True, case="exact")


def _assert_stack(res, want, n_hyp):
    assert res.images.dtype == np.complex128 and res.images.shape == want.shape and len(res.s2) == n_hyp
    for h in range(n_hyp):
        err = rel_l2(res.images[h], want[h])
        print(f"hypothesis {h}: rel L2 {err:.2e}")
        assert err < TOL, h


def test_tile_route_stack_against_the_oracle(tile_case):
    sc, hyps, want, res = tile_case
    assert res.route == "tile"
    _assert_stack(res, want, 3)
    # one chunk of 320 pulses: the 256-pulse batch boundary inside a chunk
    one = _search(sc, hyps, 90, 70, images=True, chunks=1)
    assert one.route == "tile"
    _assert_stack(one, want, 3)
    # the same fp32 terms added in fp64 in another order (as a rule every partial sum is exact, and the two stacks are equal)
    assert max(rel_l2(one.images[h], res.images[h]) for h in range(3)) < 1e-12


def test_exact_route_stack_against_the_oracle(exact_case):
    sc, hyps, want, res = exact_case
    assert res.route == "exact"
    _assert_stack(res, want, 3)
    assert _search(sc, hyps, 40, 40).route == "tile"                 # what the scene takes by itself (see _route)


def test_exact_route_by_geometry(exact_case):
    """The same pulses on 24 x 20 pixels of 17 and 21 m: a tile's corner is too far from its reference pixel for the expansion."""
    sc, hyps, _, _ = exact_case
    res = _search(sc, hyps, 24, 20, images=True)
    assert res.route == "exact"
    _assert_stack(res, ref.stack_images(sc, hyps, 24, 20), 3)
    want = ref.records(res.images)
    assert np.array_equal(res.peak, want["peak"]) and np.array_equal(res.peak_ix, want["peak_ix"]) and np.array_equal(res.peak_iy, want["peak_iy"])


@pytest.mark.parametrize("case", ["tile", "exact"])
def test_stack_equals_one_focus_call_per_hypothesis(case, tile_case, exact_case):
    """+-40 m/s in both ground directions: each hypothesis alone would compress another window; the search compresses the union."""
    import sarx
    sc, _, _, first = tile_case if case == "tile" else exact_case
    nx, ny = (90, 70) if case == "tile" else (40, 40)
    hyps = np.array([[40.0, 40.0, 0.0], [-40.0, 40.0, 0.0], [0.0, 0.0, 0.0], [40.0, -40.0, 0.0], [-40.0, -40.0, 0.0]]) + sc["v_tgt"][None, :]
    raw = sc["raw"].astype(np.complex64)
    res = _search(sc, hyps, nx, ny, raw=raw, images=True, case=case)
    assert res.route == first.route == case
    single = _search(sc, hyps[3:4], nx, ny, raw=raw, images=True, case=case)       # n_hyp = 1
    with _route(case):
        focus = [sarx.tdbp_gpu(raw, sc["pos"], sc["vel"], sc["t_start"], sc["num_samples"], v, sc["t_vec"], sc["swath"], nx, ny,
                               consts=sc["k"]) for v in hyps]
    for h in range(5):
        err = rel_l2(res.images[h], focus[h])
        print(f"{case} hypothesis {h}: rel L2 against tdbp_gpu {err:.2e}")
        assert err < KERNEL_TOL, h
    assert single.images.shape == (1, ny, nx) and rel_l2(single.images[0], focus[3]) < KERNEL_TOL
    assert len(single.s4) == 1 and single.peak[0] == ref.metrics(single.images[0])[2]


@pytest.mark.parametrize("case", ["tile", "exact"])
def test_records_are_the_fp64_sums_of_the_device_stack(case, tile_case, exact_case):
    res = (tile_case if case == "tile" else exact_case)[3]
    want = ref.records(res.images)
    for name in ("s2", "s4"):
        rel = np.abs(getattr(res, name) - want[name]) / want[name]
        print(case, name, rel)
        assert (rel < 1e-12).all(), name                            # summation order alone: n eps ~ 7e-13 for 6300 pixels
    assert np.array_equal(res.peak, want["peak"])
    assert np.array_equal(res.peak_ix, want["peak_ix"]) and np.array_equal(res.peak_iy, want["peak_iy"])
    assert np.isfinite(res.s2).all() and (res.peak > 0).all()


def test_peak_ties_go_to_the_smaller_linear_index():
    """The metric launch alone over a stack with equal maxima: in two threads, in one thread (1024 pixels apart), and a flat
    image; then one NaN that must not become the peak."""
    import sarx
    from sarx import tdbp
    mod = importlib.import_module("sarx.tdbp_search")
    ctx = sarx.default_context()
    k = tb.scaled_constants()
    nx, ny = 90, 70
    plan = tdbp.cached_plan(ctx, k, 160, tb.spotlight_window(k)[0], nx, ny)
    rng = np.random.default_rng(5)
    stack = (rng.standard_normal((4, ny, nx)) + 1j * rng.standard_normal((4, ny, nx))) * 0.1
    for h, places in enumerate(([5000, 100], [1124 + 2048, 1124], [6299, 6298, 1023])):
        for i in places:
            stack[h].ravel()[i] = 3.0 - 4.0j
    stack[2].ravel()[1023] = 4.0 + 3.0j                                # the same power from other parts
    stack[3] = 1.0 + 1.0j
    stack[3, 0, 0] = np.nan
    d_stack, d_rec = ctx.to_device(stack), ctx.alloc(4 * 32)
    try:
        _ffi = importlib.import_module("sarx._ffi")
        _ffi.check(ctx.lib.sarx_tdbp_search_metric_dev(plan.h, d_stack.ptr, 4, d_rec.ptr), ctx.h)
        rec = d_rec.download(np.uint8, (128,)).view(mod.RECORD_DTYPE)
    finally:
        d_stack.release()
        d_rec.release()
    want = ref.records(stack[:3])
    assert [(int(r["peak_ix"]), int(r["peak_iy"])) for r in rec[:3]] == [(100 % nx, 100 // nx), (1124 % nx, 1124 // nx), (1023 % nx, 1023 // nx)]
    assert np.array_equal(rec["peak"][:3], want["peak"]) and (rec["peak"][:3] == 25.0).all()
    assert np.array_equal(rec["peak_ix"][:3], want["peak_ix"]) and np.array_equal(rec["peak_iy"][:3], want["peak_iy"])
    assert (np.abs(rec["s2"][:3] - want["s2"]) <= 1e-12 * want["s2"]).all() and (np.abs(rec["s4"][:3] - want["s4"]) <= 1e-12 * want["s4"]).all()
    assert rec["peak"][3] == 2.0 and (int(rec["peak_ix"][3]), int(rec["peak_iy"][3])) == (1, 0) and np.isnan(rec["s2"][3])


def test_an_all_nan_image_has_a_nan_record_and_no_peak():
    """The metric launch alone over a 33 x 17 stack of two hypotheses: the first image all NaN - no power compares greater than the
    fold's start, so s2, s4 and the peak are NaN and the peak's place is (-1, -1) - the second finite, its record NumPy's."""
    import sarx
    from sarx import tdbp
    mod = importlib.import_module("sarx.tdbp_search")
    _ffi = importlib.import_module("sarx._ffi")
    ctx = sarx.default_context()
    k = tb.scaled_constants()
    nx, ny = 33, 17
    plan = tdbp.cached_plan(ctx, k, 160, tb.spotlight_window(k)[0], nx, ny)
    rng = np.random.default_rng(7)
    stack = rng.standard_normal((2, ny, nx)) + 1j * rng.standard_normal((2, ny, nx))
    stack[0] = complex(np.nan, np.nan)
    d_stack, d_rec = ctx.to_device(stack), ctx.alloc(2 * 32)
    try:
        _ffi.check(ctx.lib.sarx_tdbp_search_metric_dev(plan.h, d_stack.ptr, 2, d_rec.ptr), ctx.h)
        rec = d_rec.download(np.uint8, (64,)).view(mod.RECORD_DTYPE)
    finally:
        d_stack.release()
        d_rec.release()
    assert np.isnan(rec["s2"][0]) and np.isnan(rec["s4"][0]) and np.isnan(rec["peak"][0])
    assert (int(rec["peak_ix"][0]), int(rec["peak_iy"][0])) == (-1, -1)
    want = ref.records(stack[1:])
    assert (rec["peak"][1], rec["peak_ix"][1], rec["peak_iy"][1]) == (want["peak"][0], want["peak_ix"][0], want["peak_iy"][0])
    assert abs(rec["s2"][1] - want["s2"][0]) <= 1e-12 * want["s2"][0] and abs(rec["s4"][1] - want["s4"][0]) <= 1e-12 * want["s4"][0]


def test_records_are_bit_identical_with_and_without_the_stack_and_from_run_to_run(tile_case, exact_case):
    for case, (sc, hyps, _, first) in (("tile", tile_case), ("exact", exact_case)):
        nx, ny = first.images.shape[2], first.images.shape[1]
        a = _search(sc, hyps, nx, ny, case=case)
        b = _search(sc, hyps, nx, ny, case=case)
        c = _search(sc, hyps, nx, ny, images=True, case=case)
        assert a.images is None and a.route == first.route
        assert a.records.tobytes() == b.records.tobytes() == c.records.tobytes() == first.records.tobytes()
        assert np.array_equal(c.images, first.images)


def test_device_resident_raw_gives_the_same_records(exact_case):
    import sarx
    sc, hyps, _, _ = exact_case
    k = sc["k"]
    args = (sc["targets"], sc["t_vec"], sc["pos"], sc["vel"], sc["heading_deg"], sc["speed"], sc["l_ant"])
    d_raw, t0, n, v = sarx.run_physics_spotlight(*args, consts=k, device=True)
    raw = sarx.run_physics_spotlight(*args, consts=k)[0]
    common = (sc["t_vec"], sc["swath"], 40, 40)
    try:
        with _route("exact"):
            dev = sarx.tdbp_search(d_raw, sc["pos"], sc["vel"], t0, n, hyps, *common, consts=k, images=True)
            host = sarx.tdbp_search(raw, sc["pos"], sc["vel"], t0, n, hyps, *common, consts=k, images=True)
            again = sarx.tdbp_search(d_raw, sc["pos"], sc["vel"], t0, n, hyps[:2], *common, consts=k)
    finally:
        d_raw.release()
    assert dev.records.tobytes() == host.records.tobytes() and np.array_equal(dev.images, host.images)
    assert again.records.tobytes() == dev.records[:2].tobytes() and again.images is None
    assert dev.route == host.route == "exact"


def test_recovery_of_the_along_track_velocity_on_the_device():
    """The 2048-pulse scene of tests/test_tdbp_search.py, the echo from the device: sum |I|^4 peaks at the truth, the parabola
    lands within half a grid step, and tdbp_autofocus - seeded 6 m/s off along track - focuses at least as well as its seed."""
    import sarx
    sc = ref.recovery_scene()
    k = sc["k"]
    nx, ny = ref.RECOVERY_NX, ref.RECOVERY_NY
    d_raw, t0, n, v_tgt = sarx.run_physics_spotlight(sc["targets"], sc["t_vec"], sc["pos"], sc["vel"], sc["heading_deg"], sc["speed"],
                                                     sc["l_ant"], consts=k, device=True)
    try:
        hyps = ref.recovery_hyps(sc)
        res = sarx.tdbp_search(d_raw, sc["pos"], sc["vel"], t0, n, hyps, sc["t_vec"], sc["swath"], nx, ny, consts=k)
        print("s4:", " ".join(f"{x:.3e}" for x in res.s4))
        assert int(np.argmax(res.s4)) == 4 and np.array_equal(hyps[4], v_tgt)
        e = res.estimate("s4")
        print(e)
        assert not e.edge and np.linalg.norm(e.velocity - v_tgt) < 1.5
        v0 = v_tgt - np.array([6.0, 0.0, 0.0])
        v_est, img, auto = sarx.tdbp_autofocus(d_raw, sc["pos"], sc["vel"], t0, n, sc["t_vec"], sc["swath"], nx, ny, v0=v0,
                                               half_span=12.0, n=9, consts=k)
        seed = sarx.tdbp_gpu(d_raw, sc["pos"], sc["vel"], t0, n, v0, sc["t_vec"], sc["swath"], nx, ny, consts=k)
    finally:
        d_raw.release()
    p_auto, p_seed = float(ref.power(img).max()), float(ref.power(seed).max())
    print(f"autofocus: v_est {v_est}, peak power {p_auto:.4e} against {p_seed:.4e} at the seed")
    assert img.shape == (ny, nx) and len(auto.s4) == 9 and auto.images is None
    assert np.linalg.norm(v_est - v_tgt) < 1.5
    assert p_auto >= p_seed


def test_refusals():
    import sarx
    _ffi = importlib.import_module("sarx._ffi")
    k = tb.scaled_constants()
    n_s = tb.spotlight_window(k)[0]
    n_p = 8
    raw = np.zeros((n_p, n_s), np.complex64)
    pos = np.tile(np.array([0.0, -3e5, 4e5]), (n_p, 1))
    vel = np.tile(np.array([7e3, 0.0, 0.0]), (n_p, 1))
    tp = np.arange(n_p) / 5e3
    good = np.zeros((2, 3))

    def call(hyps, **kw):
        return sarx.tdbp_search(raw, pos, vel, 0.0, n_s, hyps, tp, 10.0, 8, 8, consts=k, **kw)

    ctx = sarx.default_context()
    d_raw = ctx.to_device(raw)
    try:
        for hyps in (np.zeros((0, 3)), np.zeros((_ffi.TDBP_SEARCH_MAX_HYP + 1, 3)), np.array([[0.0, np.nan, 0.0]]),
                     np.array([[0.0, 0.0, 0.0], [np.inf, 0.0, 0.0]])):
            for images in (False, True):
                with pytest.raises(sarx.SarxError) as e:
                    call(hyps, images=images)
                assert e.value.code == -1 and ("n_hyp" in str(e.value) or "non-finite" in str(e.value))
                with pytest.raises(sarx.SarxError):
                    sarx.tdbp_search(d_raw, pos, vel, 0.0, n_s, hyps, tp, 10.0, 8, 8, consts=k, images=images)
        with pytest.raises(sarx.SarxError):
            sarx.tdbp_search(raw, pos, vel, 0.0, n_s, good, tp, 0.0, 8, 8, consts=k)              # scene size
        for bad in (np.zeros(3), np.zeros((2, 2))):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError):
            sarx.tdbp_search(raw[:, :-2], pos, vel, 0.0, n_s, good, tp, 10.0, 8, 8, consts=k)
        with pytest.raises(sarx.SarxError):
            call(good, chunks=65)
        assert len(call(good).s2) == 2                                                            # and the good call goes through
        # NULL pointers and a destroyed plan, on the C ABI itself
        lib = ctx.lib
        plan = sarx.TdbpPlan(ctx, n_p, n_s, 8, 8, k)
        d_rec = ctx.alloc(64)
        a = dict(raw=d_raw.ptr, pos=pos.ctypes.data, vel=vel.ctypes.data, tp=tp.ctypes.data, hyps=good.ctypes.data, rec=d_rec.ptr)

        def dev(h, **kw):
            b = dict(a, **kw)
            return lib.sarx_tdbp_search_dev(h, b["raw"], b["pos"], b["vel"], b["tp"], 0.0, b["hyps"], 2, 10.0, None, b["rec"])

        tile = C.c_int(-5)
        assert lib.sarx_tdbp_search_route(plan.h, C.byref(tile)) == -1 and "search" in ctx.last_error()      # none run yet
        for name in a:
            assert dev(plan.h, **{name: None}) == -1 and "NULL" in ctx.last_error(), name
        assert dev(plan.h) == 0
        ctx.sync()
        assert lib.sarx_tdbp_search_route(plan.h, C.byref(tile)) == 0 and tile.value in (0, 1)
        stale = plan.h.value
        plan.close()
        assert dev(stale) == -1 and b"live" in lib.sarx_last_error(None)
        assert lib.sarx_tdbp_search_route(stale, C.byref(tile)) == -1
        assert lib.sarx_tdbp_search_set_chunks(stale, 1) == -1
        assert lib.sarx_tdbp_search_metric_dev(stale, d_raw.ptr, 1, d_rec.ptr) == -1
        host_rec = np.zeros(2, ref.RECORD_DTYPE)
        assert lib.sarx_tdbp_search_host(stale, raw.ctypes.data, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, 0.0, good.ctypes.data,
                                         2, 10.0, None, host_rec.ctypes.data) == -1
        d_rec.release()
    finally:
        d_raw.release()
