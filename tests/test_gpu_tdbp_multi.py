"""The N-receiver back-projection and the multi-baseline ATI resolver on the device (sarx.tdbp_multi,
include/sarx_tdbp_multi.h) against their fp64 NumPy restatement (tests/_tdbp_multi_numpy.py): relative L2 < 1e-4 per channel, the
pair's bar; the tile form against the exact one < 2e-6, the project's kernel-to-kernel bar; n_rx = 2 against sarx.tdbp_pair byte
for byte; the resolver's records against the restated resolver run on the downloaded device images."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_multi_numpy as ref  # noqa: E402
import _tdbp_pair_numpy as pref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
KERNEL_TOL = 2e-6
VF = (3.0, -8.0, 0.0)
# pulse ranges on the 160-pulse four-receiver scene: aligned (155 used; the fourth channel's 3.65 pulses set by hand) and not
RANGES = {3: {"aligned": ((5, 4, 0), 155), "unaligned": ((0, 3, 7), 150)},
          4: {"aligned": (ref.FIRST_4, 155), "unaligned": ((2, 0, 9, 4), 150)}}
# a grid the tile expansion takes with the longest offset 9 d = 13.9 m: |q|^2 |off| / (sqrt(3) d^2) = 5.4e-10 m for 0.26 x 0.43 m
# pixels at 4.9e5 m; three tiles by two, the lower row ragged
TILE_GRID = (10.0, 40, 24)


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _multi(sc, scene_size, nx, ny, ranges, vf=(0.0, 0.0, 0.0), channels=None, raw=None, **kw):
    import sarx
    ch = list(range(len(sc["raw"]))) if channels is None else list(channels)
    raw = [sc["raw"][c] for c in ch] if raw is None else raw
    return sarx.tdbp_multi(raw, sc["pos"], sc["vel"], [sc["rx_offsets"][c] for c in ch], sc["t_start"], sc["num_samples"], sc["t_vec"],
                           scene_size, nx, ny, vel_focus=vf, chirp_centre=sc["chirp_centre"], pulse_ranges=ranges, consts=sc["k"], **kw)


def _assert_stack(res, want, route):
    assert res.route == route
    assert res.imgs.dtype == np.complex128 and res.imgs.shape == want.shape
    for c in range(want.shape[0]):
        err = ref.rel_l2(res.imgs[c], want[c])
        print(f"channel {c}: rel L2 {err:.2e}")
        assert err < TOL, c


@pytest.mark.parametrize("vf", [(0.0, 0.0, 0.0), VF], ids=["still", "focus"])
@pytest.mark.parametrize("ranges", ["aligned", "unaligned"])
@pytest.mark.parametrize("grid", [(40, 40), (37, 21)], ids=["40x40", "37x21"])
@pytest.mark.parametrize("n_rx", [3, 4])
def test_exact_route_against_the_restatement(n_rx, grid, ranges, vf):
    """160 pulses of the scaled radar over 400 m with SARX_TDBP_TILE=0: 40 x 40, and 37 x 21 with ragged tiles in both directions.
    Unaligned ranges have every channel start and stop at another pulse inside the union loop."""
    sc = ref.four_rx_scene()
    nx, ny = grid
    first, n_used = RANGES[n_rx][ranges]
    want = ref.stack_images(sc, 400.0, nx, ny, first, n_used, vf, channels=range(n_rx))
    with _env("SARX_TDBP_TILE", "0"):
        res = _multi(sc, 400.0, nx, ny, (first, n_used), vf, channels=range(n_rx))
    _assert_stack(res, want, "exact")
    lam = sc["wavelength"]
    assert res.lags_s == pytest.approx(sc["lags"][:n_rx - 1], rel=1e-9)
    assert res.v_ambiguity == pytest.approx([lam / (4 * x) for x in sc["lags"][:n_rx - 1]], rel=1e-9)


def test_tile_route_against_the_restatement_and_the_exact_route():
    """Three receivers, 320 pulses, 315 used, on the tile grid: the library's own chunks, one chunk (a batch boundary at 256 inside
    the loop) and three chunks of 105 (chunk boundaries inside every channel's range); the exact kernel through SARX_TDBP_TILE=0."""
    sc = ref.three_rx_scene(16.0)
    size, nx, ny = TILE_GRID
    ranges = (ref.FIRST_3, ref.N_USED)
    want = ref.stack_images(sc, size, nx, ny, *ranges)
    runs = {"default": _multi(sc, size, nx, ny, ranges), "one chunk": _multi(sc, size, nx, ny, ranges, chunks=1),
            "three chunks": _multi(sc, size, nx, ny, ranges, chunks=3)}
    for got in runs.values():
        _assert_stack(got, want, "tile")
    with _env("SARX_TDBP_TILE", "0"):
        exact = _multi(sc, size, nx, ny, ranges, chunks=3)
    _assert_stack(exact, want, "exact")
    for name, got in runs.items():
        for c in range(3):
            err = ref.rel_l2(got.imgs[c], exact.imgs[c])
            print(f"tile ({name}) against exact, channel {c}: rel L2 {err:.2e}")
            assert err < KERNEL_TOL
    # the same fp32 terms added in fp64 in another order
    assert ref.rel_l2(runs["one chunk"].imgs, runs["three chunks"].imgs) < 1e-12


@pytest.mark.parametrize("vf", [(0.0, 0.0, 0.0), VF], ids=["still", "focus"])
def test_tile_route_with_four_receivers(vf):
    """The 32 KiB records of N = 4 with a channel whose lag is no whole pulse, unaligned ranges, with and without a focus velocity."""
    sc = ref.four_rx_scene()
    size, nx, ny = TILE_GRID
    first, n_used = RANGES[4]["unaligned"]
    want = ref.stack_images(sc, size, nx, ny, first, n_used, vf)
    res = _multi(sc, size, nx, ny, (first, n_used), vf)
    _assert_stack(res, want, "tile")
    with _env("SARX_TDBP_TILE", "0"):
        exact = _multi(sc, size, nx, ny, (first, n_used), vf)
    assert exact.route == "exact"
    for c in range(4):
        err = ref.rel_l2(res.imgs[c], exact.imgs[c])
        print(f"tile against exact, channel {c}: rel L2 {err:.2e}")
        assert err < KERNEL_TOL


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c128", "c64"])
@pytest.mark.parametrize("route", ["exact", "tile"])
def test_two_receivers_are_the_pair_byte_for_byte(route, dtype):
    """n_rx = 2 against sarx.tdbp_pair on the pair's own scene with the DPCA shift and a focus velocity: the same bytes."""
    import sarx
    sc = pref.stationary_scene()
    size, nx, ny = (400.0, 40, 40) if route == "exact" else TILE_GRID
    n_p = len(sc["t_vec"])
    with _env("SARX_TDBP_TILE", "0" if route == "exact" else "1"):
        pair = sarx.tdbp_pair(sc["raw"][0], sc["raw"][1], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"],
                              size, nx, ny, vel_focus=VF, chirp_centre=sc["chirp_centre"], pulse_shift=True, consts=sc["k"], dtype=dtype)
        res = sarx.tdbp_multi(sc["raw"], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"], size, nx, ny,
                              vel_focus=VF, chirp_centre=sc["chirp_centre"], pulse_ranges=((1, 0), n_p - 1), consts=sc["k"], dtype=dtype)
        auto = sarx.tdbp_multi(sc["raw"], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"], size, nx, ny,
                               vel_focus=VF, chirp_centre=sc["chirp_centre"], consts=sc["k"], dtype=dtype)     # the aligned ranges are the DPCA shift
    assert pair.route == res.route == auto.route == route
    assert res.imgs.dtype == dtype and np.abs(res.imgs).max() > 0
    assert res.imgs[0].tobytes() == pair.img1.tobytes() and res.imgs[1].tobytes() == pair.img2.tobytes()
    assert auto.imgs.tobytes() == res.imgs.tobytes()
    assert res.lags_s[0] == pair.lag_s and res.v_ambiguity[0] == pair.v_ambiguity


@pytest.mark.parametrize("route", ["exact", "tile"])
def test_permuting_two_channels_permutes_their_images(route):
    """Channels 1 and 2 exchanged in the input (raw pulses, offsets, first pulses): images 1 and 2 exchanged byte for byte, image 0
    unchanged."""
    sc = ref.four_rx_scene()
    size, nx, ny = (400.0, 37, 21) if route == "exact" else TILE_GRID
    first, n_used = RANGES[3]["unaligned"]
    with _env("SARX_TDBP_TILE", "0" if route == "exact" else "1"):
        a = _multi(sc, size, nx, ny, (first, n_used), VF, channels=(0, 1, 2))
        b = _multi(sc, size, nx, ny, ((first[0], first[2], first[1]), n_used), VF, channels=(0, 2, 1))
    assert a.route == b.route == route
    assert b.imgs[0].tobytes() == a.imgs[0].tobytes()
    assert b.imgs[1].tobytes() == a.imgs[2].tobytes() and b.imgs[2].tobytes() == a.imgs[1].tobytes()
    assert a.imgs[1].tobytes() != a.imgs[2].tobytes()


def _scratch(ctx, plan):
    n, h = C.c_uint64(), C.c_uint64()
    assert ctx.lib.sarx_tdbp_multi_scratch(plan.h, C.byref(n), C.byref(h)) == 0, ctx.last_error()
    return n.value, h.value


def test_output_forms_reruns_and_device_residency():
    """Reruns are the same bits; complex64 = the complex128 sums rounded once; device-resident raw and outputs give the host path's
    bits; a repeated call allocates nothing: the scratch holds the same bytes at the same addresses."""
    import sarx
    from sarx import tdbp as _tdbp
    sc = ref.four_rx_scene()
    ctx = sarx.default_context()
    ranges = RANGES[4]["aligned"]
    res = _multi(sc, 400.0, 37, 21, ranges)
    plan = _tdbp.cached_plan(ctx, sc["k"], len(sc["t_vec"]), sc["num_samples"], 37, 21)
    held = _scratch(ctx, plan)
    assert held[0] > 0
    again = _multi(sc, 400.0, 37, 21, ranges)
    assert again.imgs.tobytes() == res.imgs.tobytes()
    assert _scratch(ctx, plan) == held
    narrow = _multi(sc, 400.0, 37, 21, ranges, dtype=np.complex64)
    assert narrow.imgs.dtype == np.complex64 and narrow.imgs.tobytes() == res.imgs.astype(np.complex64).tobytes()
    assert _scratch(ctx, plan) == held                                 # the host staging holds both output forms from the first call
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    try:
        wide = _multi(sc, 400.0, 37, 21, ranges, raw=d_raw)
        assert wide.imgs.tobytes() == res.imgs.tobytes()
        dev = _multi(sc, 400.0, 37, 21, ranges, raw=d_raw, device_output=True)
        try:
            assert len(dev.imgs) == 4 and dev.imgs[3].shape == (21, 37)
            for c in range(4):
                assert dev.imgs[c].numpy().tobytes() == narrow.imgs[c].tobytes()
            assert dev.pair(3).img2.numpy().tobytes() == narrow.imgs[3].tobytes() and dev.pair(3).lag_s == dev.lags_s[2]
        finally:
            dev.release()
        assert _scratch(ctx, plan) == held
    finally:
        for b in d_raw:
            b.release()


def _compare_records(got, want):
    assert len(got) == len(want)
    np.testing.assert_array_equal(got["k"], want["k"])
    np.testing.assert_array_equal(got["status"], want["status"])
    assert np.max(np.abs(got["phase"] - want["phase"]), initial=0.0) <= 1e-12
    assert np.max(np.abs(got["v_los"] - want["v_los"]), initial=0.0) <= 1e-9
    assert np.max(np.abs(got["v_coarse"] - want["v_coarse"]), initial=0.0) <= 1e-9
    for f in ("cost", "cost_next"):
        fin = np.isfinite(want[f])
        np.testing.assert_array_equal(np.isfinite(got[f]), fin)
        assert np.max(np.abs(got[f][fin] - want[f][fin]), initial=0.0) <= 1e-9


def test_the_device_stack_feeds_the_gmti_chain_and_the_resolver():
    """The v_y = 16 m/s scene as a device-resident three-channel stack -> pair(1) -> sarx.gmti_detect -> resolve.  Every record
    against the restated resolver on the downloaded device images; the strongest cell has k = -1 and the true speed within 2 %,
    where the long baseline alone is off by more than its v_ambiguity.  No report is left out (tests/test_tdbp_multi.py holds
    every one of them clear of a tie)."""
    import sarx
    ctx = sarx.default_context()
    sc = ref.three_rx_scene(16.0)
    size, nx, ny = ref.GRID
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    dev = _multi(sc, size, nx, ny, None, raw=d_raw, device_output=True)        # None: the aligned ranges, derived from the offsets
    try:
        xs, ys = np.linspace(-size / 2, size / 2, nx), np.linspace(-size / 2, size / 2, ny)
        lam = sc["wavelength"]
        short = dev.pair(1)
        assert short.lag_s == pytest.approx(1.0 / sc["k"]["PRF"], rel=1e-9) and dev.lags_s[1] == pytest.approx(5.0 / sc["k"]["PRF"], rel=1e-9)
        rep = sarx.gmti_detect(short.img1, short.img2, xs, ys, wavelength_m=lam, platform_speed_mps=sc["speed"], lag_s=short.lag_s,
                               guard=(2, 2), train=(8, 8), pfa=1e-3, max_detections=4096)
        d = rep.detections
        cells = list(zip(d["i"].tolist(), d["j"].tolist()))
        assert len(cells) >= 1
        imgs = np.stack([z.numpy() for z in dev.imgs])
        for c, z in enumerate(ref.three_rx_images(16.0)):
            assert ref.rel_l2(imgs[c], z) < TOL                                # the aligned ranges were (5, 4, 0), 315
        got = dev.resolve(rep, 30.0)
        want = ref.resolve(imgs, cells, sc["lags"], lam, 30.0)
        _compare_records(got, want)
        assert np.all(got["status"] == 0)
        m = np.abs(imgs[0] - imgs[1])
        pi, pj = np.unravel_index(np.argmax(m), m.shape)
        assert (int(pi), int(pj)) in cells
        r = got[cells.index((int(pi), int(pj)))]
        truth = ref.v_los_true(sc, 16.0)
        wrapped = -lam * r["phase"][1] / (4 * np.pi * dev.lags_s[1])
        print(f"{len(cells)} reports; strongest at ({pi}, {pj}): wrapped {wrapped:.3f}, k {r['k']}, resolved {r['v_los']:.3f}, "
              f"coarse {r['v_coarse']:.3f} against {truth:.3f} m/s; cost {r['cost']:.2e}, next {r['cost_next']:.3f}")
        assert r["k"] == -1 and abs(r["v_los"] - truth) < 0.02 * truth
        assert abs(wrapped - truth) > dev.v_ambiguity[1]
        # a wider window, and the slot handed over as raw reports
        bare = np.zeros(len(cells), sarx.gmti.REPORT_DTYPE)
        bare["i"], bare["j"] = d["i"], d["j"]
        _compare_records(dev.resolve(bare, 30.0, half=2), ref.resolve(imgs, cells, sc["lags"], lam, 30.0, half=2))
        # two receivers: one baseline, k = 0, the report's own ATI speed
        two = sarx.TdbpMultiResult(dev.imgs[:2], dev.lags_s[:1], lam, dev.route, ctx)
        got2 = two.resolve(rep, 30.0)
        _compare_records(got2, ref.resolve(imgs[:2], cells, sc["lags"][:1], lam, 30.0))
        assert np.all(got2["k"] == 0) and np.all(got2["cost"] == 0.0)
        assert np.max(np.abs(got2["v_los"] - d["v_los_mps"])) <= 1e-9
    finally:
        dev.release()
        for b in d_raw:
            b.release()


def test_resolve_takes_a_device_slot_and_raises_on_an_overflowed_one():
    """TdbpMultiResult.resolve on a host stack of noise: a slot that lies on the device (its capacity given) gives the records of the
    same reports handed over from the host, and those of the restated resolver; an overflow flag or a count above the capacity, on the
    host or on the device, raises GmtiOverflowError and returns nothing."""
    import sarx
    from sarx import slot
    ctx = sarx.default_context()
    rng = np.random.default_rng(3)
    imgs = (rng.standard_normal((3, 21, 37)) + 1j * rng.standard_normal((3, 21, 37))).astype(np.complex64)
    lags, lam, md = (2e-4, -1e-3), 0.03, 8
    res = sarx.TdbpMultiResult(imgs, lags, lam, "exact", ctx)
    cells = [(0, 0), (10, 18), (20, 36)]
    rep = np.zeros(len(cells), slot.REPORT_DTYPE)
    rep["i"], rep["j"] = zip(*cells)
    want = ref.resolve(imgs, cells, lags, lam, 40.0)
    host = res.resolve(rep, 40.0)
    _compare_records(host, want)
    held = [ctx.to_device(slot.encode(rep, md))]
    try:
        dev = res.resolve(held[0], 40.0, max_detections=md)
        assert dev.tobytes() == host.tobytes()
        with pytest.raises(ValueError, match="capacity"):
            res.resolve(held[0], 40.0)
        flagged, counted = slot.encode(rep, md), slot.encode(rep, md)
        flagged[4:8].view("<u4")[0] = 1
        counted[:4].view("<u4")[0] = md + 1
        for raw in (flagged, counted):
            with pytest.raises(sarx.GmtiOverflowError):
                res.resolve(raw, 40.0, max_detections=md)
            held.append(ctx.to_device(raw))
            with pytest.raises(sarx.GmtiOverflowError):
                res.resolve(held[-1], 40.0, max_detections=md)
    finally:
        for b in held:
            b.release()


def test_refusals_with_a_live_plan():
    """What needs the plan's pulse count: pulse ranges past the end, a zero vel_tx row; the route query before any multi call; the
    resolver's device arguments."""
    import sarx
    from sarx.tdbp_multi import resolve_params
    sc = ref.four_rx_scene()
    with pytest.raises(sarx.SarxError, match="outside"):
        _multi(sc, 400.0, 40, 40, ((1, 0, 0, 0), 160))
    vel = sc["vel"].copy()
    vel[77] = 0.0
    with pytest.raises(sarx.SarxError, match="vel_tx row 77"):
        _multi(dict(sc, vel=vel), 400.0, 40, 40, RANGES[4]["aligned"])
    with pytest.raises(ValueError, match="whole pulses"):
        _multi(sc, 400.0, 40, 40, None)                                        # the fourth channel lies 3.65 pulses off
    ctx = sarx.default_context()
    plan = sarx.TdbpPlan(ctx, 16, 256, 8, 8, sc["k"])
    try:
        tile = C.c_int(7)
        assert ctx.lib.sarx_tdbp_multi_route(plan.h, C.byref(tile)) == -1 and tile.value == 7
        assert "multi call" in ctx.last_error()
        assert _scratch(ctx, plan) == (0, 0)
    finally:
        plan.close()
    prm = resolve_params((2e-4, 1e-3), 0.03, 30.0, 1, 8)
    img, slot, rec = ctx.to_device(np.zeros(3 * 64, np.complex64)), ctx.to_device(np.zeros(16 + 8 * 48, np.uint8)), ctx.alloc(8 * 64)
    try:
        f = ctx.lib.sarx_tdbp_multi_resolve_dev
        assert f(ctx.h, C.byref(prm), img.ptr, 8, 8, slot.ptr, rec.ptr) == 0
        for args, word in (((None, 8, 8, slot.ptr, rec.ptr), "NULL"), ((img.ptr, 8, 8, None, rec.ptr), "NULL"),
                           ((img.ptr, 8, 8, slot.ptr, None), "NULL"), ((img.ptr, 0, 8, slot.ptr, rec.ptr), "size"),
                           ((img.ptr, 8, -1, slot.ptr, rec.ptr), "size"), ((img.ptr, (1 << 20) + 1, 8, slot.ptr, rec.ptr), "size"),
                           ((img.ptr + 4, 8, 8, slot.ptr, rec.ptr), "misaligned"),
                           ((img.ptr, 8, 8, slot.ptr + 4, rec.ptr), "misaligned"), ((img.ptr, 8, 8, slot.ptr, rec.ptr + 4), "misaligned"),
                           ((img.ptr, 8, 8, slot.ptr, slot.ptr + 8), "overlap"), ((img.ptr, 8, 8, slot.ptr, img.ptr + 64), "overlap")):
            assert f(ctx.h, C.byref(prm), *args) == -1 and word in ctx.last_error(), (args, ctx.last_error())
        assert f(ctx.h, None, img.ptr, 8, 8, slot.ptr, rec.ptr) == -1 and "NULL" in ctx.last_error()
        ctx.sync()
    finally:
        for b in (img, slot, rec):
            b.release()
