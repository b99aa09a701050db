"""The focus-velocity search on the two-receiver back-projection on the device (sarx.tdbp_pair_search,
include/sarx_tdbp_pair_search.h).  Every chip against its fp64 NumPy restatement (tests/_tdbp_pair_search_numpy.py): relative
L2 < 1e-4 per chip and channel, the project's bar; against sarx.tdbp_pair(vel_focus = v_h) at the same pixels < 2e-6, the bar of
the search against tdbp_gpu - and the same bits on the exact route when both run the same pulse chunks.  Records, k_best and the
interferogram against NumPy on the device's own chips.  Echoes come from oracle.csa_oracle.echo_bistatic, cast to complex64."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import tdbp_oracle as tb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_pair_numpy as pref  # noqa: E402
import _tdbp_pair_search_dev as dev  # noqa: E402
import _tdbp_pair_search_numpy as ref  # noqa: E402
from _guard import GuardedBuffer  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
KERNEL_TOL = 2e-6
NX, NY = 90, 70
HYPS = np.array([[0.0, 0.0, 0.0], [3.0, -8.0, 0.0], [9.0, 0.0, 0.0]])
# (i, j) = (row, column): the two corners, the middle, two whose chips overlap, and one outside the grid
PLACES = [(0, 0), (NY - 1, NX - 1), (35, 45), (30, 40), (33, 44), (NY, 5)]


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ[name]
            else:
                os.environ[name] = old


def _reports(places):
    from sarx import slot
    rep = np.zeros(len(places), slot.REPORT_DTYPE)
    rep["i"], rep["j"] = [p[0] for p in places], [p[1] for p in places]
    return rep


def _search(sc, scene_size, shift, places, hyps, chip, source="dpca", raw=None, **kw):
    import sarx
    raw = sc["raw"] if raw is None else raw
    return sarx.tdbp_pair_search(raw[0], raw[1], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"],
                                 scene_size, NX, NY, _reports(places) if isinstance(places, list) else places, hyps, chip=chip, source=source,
                                 chirp_centre=sc["chirp_centre"], pulse_shift=shift, consts=sc["k"], **kw)


def _pair(sc, scene_size, shift, vf, chunks):
    import sarx
    return sarx.tdbp_pair(sc["raw"][0], sc["raw"][1], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"],
                          scene_size, NX, NY, vel_focus=vf, chirp_centre=sc["chirp_centre"], pulse_shift=shift, consts=sc["k"], chunks=chunks)


def _assert_chips(res, sc, scene_size, shift, places, hyps, chip, pairs, same_bits):
    """Every chip of every report inside the grid against the restatement and against the whole-grid pair images `pairs` [n_hyp] of
    the same focus velocities; a report outside the grid has k_best = -1 and NaN everywhere.  Returns the worst figures."""
    cx, cy = chip
    worst_ref, worst_pair = 0.0, 0.0
    for r, (i, j) in enumerate(places):
        o = ref.chip_origin(i, j, NX, NY, cx, cy)
        if o is None:
            assert res.k_best[r] == -1 and np.isnan(res.s4[r]).all() and np.isnan(res.chips[r]).all()
            continue
        assert (res.x0[r], res.y0[r]) == o and res.k_best[r] >= 0
        for h, vf in enumerate(hyps):
            want = ref.chip_images(sc, scene_size, NX, NY, shift, o[0], o[1], cx, cy, vf)
            for c, img in enumerate((pairs[h].img1, pairs[h].img2)):
                got = res.chips[r, h, c]
                e_ref = pref.rel_l2(got, want[c])
                whole = img[o[1]:o[1] + cy, o[0]:o[0] + cx]
                e_pair = pref.rel_l2(got, whole)
                worst_ref, worst_pair = max(worst_ref, e_ref), max(worst_pair, e_pair)
                assert e_ref < TOL, (r, h, c, e_ref)
                assert e_pair < KERNEL_TOL, (r, h, c, e_pair)
                if same_bits:
                    assert got.tobytes() == np.ascontiguousarray(whole).tobytes(), (r, h, c, e_pair)
    print(f"chips against the restatement: worst rel L2 {worst_ref:.2e}; against tdbp_pair at the same pixels: {worst_pair:.2e}")
    return worst_ref, worst_pair


def _assert_records(res, source):
    """Records, best and interferogram against fp64 NumPy on the device's OWN chips: s2 and s4 to 1e-12 (another summation order),
    the peak and every index exact; the interferogram to 1e-12 of sum |I0| |I1| over its pixels."""
    for r in range(len(res)):
        if res.k_best[r] < 0:
            continue
        b = ref.best(res.chips[r], int(res.x0[r]), int(res.y0[r]), source)
        for h, (s2, s4, pk, ix, iy) in enumerate(b["records"]):
            g = res.records[r, h]
            assert abs(g["s2"] - s2) <= 1e-12 * s2 and abs(g["s4"] - s4) <= 1e-12 * s4, (r, h)
            assert (g["peak"], g["peak_ix"], g["peak_iy"]) == (pk, ix, iy), (r, h)
        kb = int(np.argmax(res.s4[r]))                               # the device's own sums; the first of equal maxima
        g = res.best[r]
        assert g["k_best"] == kb and g["reserved"] == 0
        assert (g["peak_ix"], g["peak_iy"]) == (res.records[r, kb]["peak_ix"], res.records[r, kb]["peak_iy"])
        assert g["s4_best"] == res.s4[r, kb]
        assert g["s4_prev"] == (res.s4[r, kb - 1] if kb > 0 else -1.0) and g["s4_next"] == (res.s4[r, kb + 1] if kb + 1 < res.s4.shape[1] else -1.0)
        if b["k_best"] == kb:
            assert abs(res.interf[r] - b["interf"]) <= 1e-12 * b["interf_scale"], r
            assert abs(g["p0"] - b["p0"]) <= 1e-14 * b["p0"] and abs(g["p1"] - b["p1"]) <= 1e-14 * b["p1"]


_pairs = {}


def _pairs_of(key, sc, scene_size, shift, hyps, chunks):
    """The whole-grid pair images of every hypothesis, once per (scene, shift, chunks, switch)."""
    key = (key, shift, chunks, os.environ.get("SARX_TDBP_TILE"))
    if key not in _pairs:
        _pairs[key] = [_pair(sc, scene_size, shift, vf, chunks) for vf in hyps]
    return _pairs[key]


def _set_chunks(sc, chunks):
    """tdbp_pair(chunks=...) leaves its number on the shared plan; set here for the search, whose wrapper does not touch it."""
    import sarx
    from sarx import tdbp as _tdbp
    ctx = sarx.default_context()
    plan = _tdbp.cached_plan(ctx, sc["k"], len(sc["t_vec"]), sc["num_samples"], NX, NY)
    assert ctx.lib.sarx_tdbp_search_set_chunks(plan.h, chunks) == 0


@pytest.mark.parametrize("chip", [(16, 16), (40, 24)], ids=["16x16", "40x24"])
@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("forced", [False, True], ids=["geometry", "switch"])
def test_exact_route_against_the_restatement_and_the_pair(forced, shift, chip):
    """mover_scene(): 320 pulses, 90 x 70 over 360 m, whose 4 and 5 m pixels the tile expansion cannot take - and again with
    SARX_TDBP_TILE=0.  Three hypotheses, one of them zero; five chunks of 64 pulses for the search and for the pair it is held to, so
    every partial sum is the same sum: the chips are the pair's images at the same pixels bit for bit.  Measured: against the
    restatement at most 1.3e-5 (40 x 24) and 6.3e-6 (16 x 16), against the pair 0."""
    sc = pref.mover_scene()
    with _env("SARX_TDBP_TILE", "0" if forced else None):
        pairs = _pairs_of("mover", sc, 360.0, shift, HYPS, 5)
        assert all(p.route == "exact" for p in pairs)
        _set_chunks(sc, 5)
        res = _search(sc, 360.0, shift, PLACES, HYPS, chip, chips=True)
    assert res.route == "exact" and res.chips.shape == (len(PLACES), 3, 2, chip[1], chip[0])
    assert res.lag_s == pytest.approx(sc["lag"], rel=1e-9)
    _assert_chips(res, sc, 360.0, shift, PLACES, HYPS, chip, pairs, same_bits=True)
    _assert_records(res, ref.DPCA)


@pytest.fixture(scope="module")
def native():
    """batch_constants(): 22004 samples per pulse, 320 pulses, two scatterers and a mover on 90 x 70 pixels over 90 m: the tile
    route by geometry (the scene of tests/test_gpu_tdbp_pair.py)."""
    return pref.scene(320, tb.batch_constants(), [(-20.0, 11.0, 30.0), (31.0, 33.0, 45.0)], [(8.0, -3.0, 20.0, (2.0, 6.0, 0.0))])


@pytest.mark.parametrize("chip", [(16, 16), (40, 24)], ids=["16x16", "40x24"])
@pytest.mark.parametrize("chunks,shift", [(10, True), (1, False)], ids=["ten-chunks-shift", "one-chunk-noshift"])
def test_tile_route_against_the_restatement_and_the_pair(native, chunks, shift, chip):
    """Ten chunks of 32 pulses, and one chunk of 320 across the 256-pulse batch boundary.  The chip's tiles are not the grid's, so a
    pixel is expanded about another reference pixel than in the pair's launch: the two agree to the kernel bar, not to the bit.
    Measured: against the restatement at most 4.8e-6, against the pair 3.1e-7, the tile search against the exact search 2.8e-8."""
    sc = native
    hyps = np.array([[0.0, 0.0, 0.0], [2.0, 6.0, 0.0], [-4.0, 0.0, 0.0]])
    pairs = _pairs_of("native", sc, 90.0, shift, hyps, chunks)
    assert all(p.route == "tile" for p in pairs)
    _set_chunks(sc, chunks)
    res = _search(sc, 90.0, shift, PLACES, hyps, chip, chips=True)
    assert res.route == "tile"
    _assert_chips(res, sc, 90.0, shift, PLACES, hyps, chip, pairs, same_bits=False)
    _assert_records(res, ref.DPCA)
    with _env("SARX_TDBP_TILE", "0"):
        exact = _search(sc, 90.0, shift, PLACES, hyps, chip, chips=True)
    assert exact.route == "exact"
    inside = res.k_best >= 0
    err = pref.rel_l2(res.chips[inside], exact.chips[inside])
    print(f"tile against exact: rel L2 {err:.2e}")
    assert err < KERNEL_TOL


@pytest.fixture(scope="module")
def mover_runs():
    """The mover scene with chips 37 x 21 (no multiple of anything), both sources, the library's own chunk count."""
    sc = pref.mover_scene()
    _set_chunks(sc, 0)
    return sc, {src: _search(sc, 360.0, True, PLACES, HYPS, (37, 21), src, chips=True) for src in ("dpca", "ch0")}


@pytest.mark.parametrize("source", ["dpca", "ch0"])
def test_records_and_best_against_numpy_on_the_devices_own_chips(mover_runs, source):
    _, runs = mover_runs
    res = runs[source]
    _assert_records(res, source)
    assert res.chips.tobytes() == runs["dpca"].chips.tobytes()          # the source changes what is folded, not what is imaged
    with pytest.raises(ValueError, match="uniform line"):            # the parabola is TdbpSearchResult.estimate's: these three are on no line
        res.estimate()
    v = res.v_los()
    assert v.shape == (len(PLACES),) and np.isnan(v[-1]) and np.isfinite(v[:-1]).all()


def test_reruns_are_the_same_bits_with_and_without_the_chips(mover_runs):
    sc, runs = mover_runs
    again = _search(sc, 360.0, True, PLACES, HYPS, (37, 21), chips=True)
    bare = _search(sc, 360.0, True, PLACES, HYPS, (37, 21))
    assert bare.chips is None
    for got in (again, bare):
        assert got.records.tobytes() == runs["dpca"].records.tobytes() and got.best.tobytes() == runs["dpca"].best.tobytes()
    assert again.chips.tobytes() == runs["dpca"].chips.tobytes()


def test_constructed_ties():
    """Hypotheses (a, a, b, b): the chips of equal velocities are the same bits, so s4 ties within each pair and k_best is the first of
    the winning pair with s4_next = s4_best.  Pulses of zeros: every power is 0, so every s4 ties (k_best 0) and every pixel ties
    for the peak (the chip's first pixel)."""
    sc = pref.mover_scene()
    hyps = np.array([[9.0, 0.0, 0.0], [9.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    res = _search(sc, 360.0, True, [(35, 45)], hyps, (16, 16), chips=True)
    assert res.chips[0, 0].tobytes() == res.chips[0, 1].tobytes() and res.chips[0, 2].tobytes() == res.chips[0, 3].tobytes()
    assert res.s4[0, 0] == res.s4[0, 1] and res.s4[0, 2] == res.s4[0, 3] and res.s4[0, 0] != res.s4[0, 2]
    assert res.k_best[0] in (0, 2) and res.k_best[0] == int(np.argmax(res.s4[0]))
    assert res.best["s4_next"][0] == res.best["s4_best"][0]
    zeros = [np.zeros_like(r) for r in sc["raw"]]
    res = _search(sc, 360.0, True, [(35, 45), (0, 0)], hyps, (16, 16), raw=zeros)
    assert np.all(res.s4 == 0) and np.all(res.peak == 0) and list(res.k_best) == [0, 0]
    assert list(res.best["s4_prev"]) == [-1.0, -1.0] and list(res.best["s4_next"]) == [0.0, 0.0]
    assert np.all(res.records["peak_ix"] == res.x0[:, None]) and np.all(res.records["peak_iy"] == res.y0[:, None])
    assert list(zip(res.peak_ix, res.peak_iy)) == [(37, 27), (0, 0)] and np.all(res.interf == 0)


def test_a_nan_channel_leaves_nan_records_and_no_peak():
    """The 160-pulse scene with every sample of channel 0 NaN, one report, a 16 x 16 chip, two hypotheses: channel 0's chips are NaN,
    so is every DPCA power, and no pixel becomes the peak.  The records are what the restatement says of the device's own chips;
    of NaN sums alone the first hypothesis is the best, and what hangs on the peak is NaN."""
    sc = pref.stationary_scene()
    hyps = np.array([[0.0, 0.0, 0.0], [3.0, -8.0, 0.0]])
    raw = [np.full_like(sc["raw"][0], complex(np.nan, np.nan)), sc["raw"][1]]
    _set_chunks(sc, 0)
    res = _search(sc, 360.0, True, [(35, 45)], hyps, (16, 16), "dpca", raw=raw, chips=True)
    assert len(res) == 1 and np.isnan(res.chips[0, :, 0]).all() and np.isfinite(res.chips[0, :, 1]).all()
    for h in range(2):
        s2, s4, pk, ix, iy = ref.record(res.chips[0, h], int(res.x0[0]), int(res.y0[0]), ref.DPCA)
        g = res.records[0, h]
        assert np.isnan([s2, s4, pk]).all() and (ix, iy) == (-1, -1)
        assert np.isnan([g["s2"], g["s4"], g["peak"]]).all() and (g["peak_ix"], g["peak_iy"]) == (ix, iy), h
    g = res.best[0]
    assert g["k_best"] == 0 and g["s4_prev"] == -1.0 and (g["peak_ix"], g["peak_iy"]) == (-1, -1)
    assert np.isnan([g[f] for f in ("s4_best", "interf_re", "interf_im", "p0", "p1")]).all()


def test_device_resident_raw_slot_and_outputs_and_the_host_entry_point(mover_runs):
    """Device raw and a device slot through the wrapper, and sarx_tdbp_pair_search_host on host memory, give the bits of the host
    arrays through the wrapper; the host entry point leaves the records of a report outside the grid as they were."""
    import sarx
    from sarx import tdbp as _tdbp
    sc, runs = mover_runs
    want = runs["dpca"]
    ctx = sarx.default_context()
    md = 9
    slot = dev.slot_of(PLACES, md)
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    d_slot = ctx.to_device(slot)
    try:
        got = _search(sc, 360.0, True, d_slot, HYPS, (37, 21), raw=d_raw, chips=True, max_detections=md)
        assert got.records.tobytes() == want.records.tobytes() and got.best.tobytes() == want.best.tobytes() and got.chips.tobytes() == want.chips.tobytes()
        assert d_slot.download(np.uint8, (slot.size,)).tobytes() == slot.tobytes()      # the slot is only read
    finally:
        for b in (*d_raw, d_slot):
            b.release()
    plan = _tdbp.cached_plan(ctx, sc["k"], len(sc["t_vec"]), sc["num_samples"], NX, NY)
    n = len(PLACES)
    rec = np.full((md, 3, 32), 0xFF, np.uint8)
    best = np.full((md, 80), 0xFF, np.uint8)
    chips = np.full((md, 3 * 2 * 21 * 37 * 16), 0xFF, np.uint8)
    raw = [np.ascontiguousarray(r) for r in sc["raw"]]
    rc = dev.call(ctx.lib, "sarx_tdbp_pair_search_host", plan, sc, 360.0, True, HYPS, raw[0].ctypes.data, raw[1].ctypes.data, slot.ctypes.data,
                  md, (37, 21), "dpca", rec.ctypes.data, best.ctypes.data, chips.ctypes.data)
    assert rc == 0, ctx.last_error()
    inside = want.k_best >= 0
    assert rec[:n][inside].tobytes() == want.records[inside].tobytes() and best[:n][inside].tobytes() == want.best[inside].tobytes()
    assert chips[:n][inside].tobytes() == want.chips[inside].tobytes()
    assert best[n - 1, :4].view("<i4")[0] == -1 and np.all(best[n - 1, 4:] == 0xFF) and np.all(rec[n - 1] == 0xFF) and np.all(chips[n - 1] == 0xFF)
    assert np.all(rec[n:] == 0xFF) and np.all(best[n:] == 0xFF) and np.all(chips[n:] == 0xFF)


@pytest.mark.parametrize("case", ["overflow", "count-beyond-capacity", "count-zero"])
def test_an_unusable_or_empty_slot_writes_nothing(case):
    """Poisoned outputs stay poison: an overflowed slot, a count beyond the capacity, and no report at all.  The wrapper raises
    GmtiOverflowError for the first two and returns empty arrays for the third."""
    import sarx
    from sarx import tdbp as _tdbp
    sc = pref.mover_scene()
    ctx = sarx.default_context()
    md = 4
    count, overflow = {"overflow": (3, 1), "count-beyond-capacity": (5, 0), "count-zero": (0, 0)}[case]
    slot = dev.slot_of(PLACES[:3], md, count=count, overflow=overflow)
    plan = _tdbp.cached_plan(ctx, sc["k"], len(sc["t_vec"]), sc["num_samples"], NX, NY)
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    d_slot = ctx.to_device(slot)
    outs = [GuardedBuffer(ctx, n) for n in (md * 3 * 32, md * 80, md * 3 * 2 * 16 * 16 * 16)]
    try:
        for o in outs:
            o.poison()
        rc = dev.call(ctx.lib, "sarx_tdbp_pair_search_dev", plan, sc, 360.0, True, HYPS, d_raw[0].ptr, d_raw[1].ptr, d_slot.ptr, md, (16, 16),
                      "dpca", outs[0].ptr, outs[1].ptr, outs[2].ptr)
        assert rc == 0, ctx.last_error()
        ctx.sync()
        for o in outs:
            assert np.all(o.download() == 0xFF) and not o.check_zones()
        if case == "count-zero":
            res = _search(sc, 360.0, True, d_slot, HYPS, (16, 16), raw=d_raw, chips=True, max_detections=md)
            assert len(res) == 0 and res.s4.shape == (0, 3) and res.chips.shape == (0, 3, 2, 16, 16)
        else:
            with pytest.raises(sarx.GmtiOverflowError):
                _search(sc, 360.0, True, d_slot, HYPS, (16, 16), raw=d_raw, max_detections=md)
    finally:
        for b in (*d_raw, d_slot, *outs):
            b.release()


def test_refusals_with_a_live_plan():
    """What needs the plan: pulse ranges past its pulse count, a chip larger than its grid, a zero vel_tx row; the partial sums past
    the cap, with the numbers; and the route query before any search."""
    import sarx
    from sarx.tdbp_pair import pair_params
    from sarx.tdbp_pair_search import search_params
    ctx = sarx.default_context()
    k = tb.scaled_constants()
    n_p, n_s = 16, 256
    plan = sarx.TdbpPlan(ctx, n_p, n_s, 64, 64, k)
    raw = ctx.alloc(n_p * n_s * 8)
    md = 1000
    slot = ctx.to_device(dev.slot_of([], md))
    outs = [ctx.alloc(n) for n in (md * 64 * 32, md * 80)]
    pos, vel, tp = np.ones((n_p, 3)), np.ones((n_p, 3)), np.arange(float(n_p))
    hyps = np.zeros((64, 3))
    try:
        tile = C.c_int(7)
        assert ctx.lib.sarx_tdbp_pair_search_route(plan.h, C.byref(tile)) == -1 and tile.value == 7
        assert "pair search" in ctx.last_error()

        def call(prm=None, sp=None, vel_=vel, md_=4):
            prm = prm or pair_params(n_p, (-1.0, 1.0), 0.0, True)
            sp = sp or search_params((16, 16), 3, "dpca")
            return ctx.lib.sarx_tdbp_pair_search_dev(plan.h, raw.ptr, raw.ptr, pos.ctypes.data, vel_.ctypes.data, tp.ctypes.data, 0.0, 100.0,
                                                     C.byref(prm), hyps.ctypes.data, slot.ptr + 16, slot.ptr, md_, C.byref(sp), outs[0].ptr,
                                                     outs[1].ptr, None)

        assert call(prm=pair_params(n_p, (-1.0, 1.0), 0.0, ((1, 0), n_p))) == -1 and "outside" in ctx.last_error()
        assert call(sp=search_params((65, 16), 3, "dpca")) == -1 and "chip" in ctx.last_error()
        plan_small = sarx.TdbpPlan(ctx, n_p, n_s, 12, 40, k)
        try:
            sp = search_params((16, 16), 3, "dpca")
            prm = pair_params(n_p, (-1.0, 1.0), 0.0, True)
            rc = ctx.lib.sarx_tdbp_pair_search_dev(plan_small.h, raw.ptr, raw.ptr, pos.ctypes.data, vel.ctypes.data, tp.ctypes.data, 0.0, 100.0,
                                                   C.byref(prm), hyps.ctypes.data, slot.ptr + 16, slot.ptr, 4, C.byref(sp), outs[0].ptr, outs[1].ptr, None)
            assert rc == -1 and "chip 16 x 16 is larger than the grid 40 x 12" in ctx.last_error()
        finally:
            plan_small.close()
        v0 = vel.copy()
        v0[7] = 0.0
        assert call(vel_=v0) == -1 and "vel_tx row 7" in ctx.last_error()
        # 1000 reports x 64 hypotheses x 64 x 64 pixels x 2 channels x 16 bytes = 7.8 GiB per chunk: refused before anything is allocated
        assert call(sp=search_params((64, 64), 64, "dpca"), md_=md) == -1
        msg = ctx.last_error()
        assert "partial sums" in msg and "max_detections 1000" in msg and "n_hyp 64" in msg and str(1000 * 64 * 2 * 4096 * 16) in msg and str(256 << 20) in msg
        assert ctx.lib.sarx_tdbp_pair_search_route(plan.h, C.byref(tile)) == -1 and tile.value == 7       # still no search ran
    finally:
        for b in (raw, slot, *outs):
            b.release()
        plan.close()


def test_end_to_end_pair_detect_search_on_the_device_slot():
    """The 2048-pulse scene (a mover at (495, 0) m with velocity (9, 10, 0) m/s): tdbp_pair(device_output=True) -> the DPCA plane ->
    CFAR and refine into a device slot -> tdbp_pair_search on that slot, 24 x 24 chips, nine hypotheses (9 + s, 0, 0), s = -12 .. 12
    in steps of 3.  The mover's report (the strongest DPCA cell) has k_best at s = 0, the parabola's vertex within 3 m/s of it, and
    v_los() within 5 % of the truth.  The restatement on the CPU has the vertex at -0.6 m/s and v_los 7.43 of 7.47 m/s.  Measured on
    the device: 25 reports, exact route, sum |D|^4 x 1e-21 = 5.92 7.71 9.97 11.85 12.36 11.16 8.96 6.85 5.43 (the CPU's digits), k_best 4,
    along track 8.39 m/s of 9, v_los 7.431 of 7.468 m/s."""
    import sarx
    from sarx import gmti
    ctx = sarx.default_context()
    sc = ref.long_scene()
    nx, ny, size = ref.LONG_GRID
    assert (nx, ny) == (NX, NY)
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    pair = sarx.tdbp_pair(d_raw[0], d_raw[1], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"], size, nx, ny,
                          chirp_centre=sc["chirp_centre"], pulse_shift=True, consts=sc["k"], device_output=True)
    params = gmti.GmtiParams(guard=(2, 2), train=(8, 8), pfa=1e-3, max_detections=256, lag_s=pair.lag_s)
    n = nx * ny
    planes = {name: ctx.alloc(n * 4) for name in ("ati_phase", "slc1_mag", "dpca_mag")}
    slot = ctx.alloc(params.slot_bytes())
    try:
        ctx.ati_dpca(pair.img1, pair.img2, n, 0.0, planes)
        gmti.enqueue(ctx, planes["dpca_mag"].ptr, pair.img1.ptr, pair.img2.ptr, ny, nx, params, 0.0, slot.ptr)
        hyps = sarx.tdbp_velocity_line((ref.LONG_MOVER_V[0], 0.0, 0.0), (1.0, 0.0, 0.0), 12.0, 9)
        res = sarx.tdbp_pair_search(d_raw[0], d_raw[1], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"],
                                    size, nx, ny, slot, hyps, chip=(24, 24), chirp_centre=sc["chirp_centre"], pulse_shift=True, detect=params,
                                    consts=sc["k"])
        rep = gmti.fetch_slot(ctx, slot.ptr, params.max_detections)
        reports = sarx.slot.reports(rep)
        mag = planes["dpca_mag"].download(np.float32, (ny, nx))
    finally:
        pair.release()
        for b in (*d_raw, slot, *planes.values()):
            b.release()
    assert len(res) == len(reports) >= 1
    pi, pj = np.unravel_index(np.argmax(mag), mag.shape)
    assert (int(pi), int(pj)) == ref.LONG_PEAK
    r = int(np.flatnonzero((reports["i"] == pi) & (reports["j"] == pj))[0])
    est = res.estimate()[r]
    truth = pref.v_los_true(sc, pref.MOVER_AT, ref.LONG_MOVER_V)
    print(f"{len(res)} reports, route {res.route}; the mover's: s4 x 1e-21 " + " ".join(f"{v * 1e-21:.2f}" for v in res.s4[r]) +
          f", k_best {res.k_best[r]}, along track {est.velocity[0]:.2f} m/s (truth {ref.LONG_MOVER_V[0]}), v_los {res.v_los()[r]:.3f} of {truth:.3f} m/s")
    assert res.k_best[r] == 4 and not est.edge
    assert abs(est.velocity[0] - ref.LONG_MOVER_V[0]) < 3.0
    assert abs(res.v_los()[r] - truth) < 0.05 * truth
