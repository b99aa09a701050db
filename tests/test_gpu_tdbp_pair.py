"""The two-receiver back-projection on the device (sarx.tdbp_pair, include/sarx_tdbp_pair.h) against its fp64 NumPy restatement
(tests/_tdbp_pair_numpy.py): relative L2 < 1e-4 per channel, the bar of tests/test_gpu_tdbp.py; against the existing focus
(sarx.tdbp_gpu) < 2e-6, the project's kernel-to-kernel bar.  Echoes come from oracle.csa_oracle.echo_bistatic, cast to complex64.
Both forms of the geometry are held to the same bars: the exact one, and the tile-expanded one against it to 2e-6."""
import contextlib
import os
import sys

import numpy as np
import pytest

from oracle import tdbp_oracle as tb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmti_numpy as gref  # noqa: E402
import _tdbp_pair_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
KERNEL_TOL = 2e-6
VF = (3.0, -8.0, 0.0)


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


def _pair(sc, scene_size, nx, ny, shift, vf=(0.0, 0.0, 0.0), raw=None, **kw):
    import sarx
    raw = sc["raw"] if raw is None else raw
    return sarx.tdbp_pair(raw[0], raw[1], sc["pos"], sc["vel"], sc["rx_offsets"], sc["t_start"], sc["num_samples"], sc["t_vec"], scene_size,
                          nx, ny, vel_focus=vf, chirp_centre=sc["chirp_centre"], pulse_shift=shift, consts=sc["k"], **kw)


def _assert_pair(res, want, route="exact"):
    assert res.route == route
    assert res.img1.dtype == np.complex128 and res.img1.shape == want[0].shape
    for c, img in enumerate((res.img1, res.img2)):
        err = ref.rel_l2(img, want[c])
        print(f"channel {c}: rel L2 {err:.2e}")
        assert err < TOL, c


@pytest.mark.parametrize("vf", [(0.0, 0.0, 0.0), VF], ids=["still", "focus"])
@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("grid", [(40, 40), (24, 20)], ids=["40x40-forced", "24x20-geometry"])
def test_exact_route_against_the_restatement(grid, shift, vf):
    """160 pulses of the scaled radar over 400 m: 40 x 40 with the focus tests' switch SARX_TDBP_TILE=0, and 24 x 20, whose 17 and
    21 m pixels the tile expansion cannot take.  Both pulse-range settings (the DPCA shift has the two channels start and stop one
    pulse apart inside the union loop, five chunks of 32), vel_focus zero and not."""
    sc = ref.stationary_scene()
    nx, ny = grid
    want = ref.images(sc, 400.0, nx, ny, shift, vf)
    with _env("SARX_TDBP_TILE", "0"):
        res = _pair(sc, 400.0, nx, ny, shift, vf)
    _assert_pair(res, want)
    assert res.lag_s == pytest.approx(sc["lag"], rel=1e-9) and res.v_ambiguity == pytest.approx(sc["k"]["C"] / sc["k"]["FC"] / (4 * sc["lag"]), rel=1e-9)


@pytest.fixture(scope="module")
def native():
    """batch_constants(): 22004 samples per pulse, a 12000-tap reference, 320 pulses, two scatterers and a mover on 90 x 70
    pixels over 90 m: ragged tiles, the tile route by geometry (5 u^4 / 128 d = 1e-13 m, |q|^2 |off| / (sqrt(3) d^2) = 6.5e-10 m)."""
    sc = ref.scene(320, tb.batch_constants(), [(-20.0, 11.0, 30.0), (31.0, 33.0, 45.0)], [(8.0, -3.0, 20.0, (2.0, 6.0, 0.0))])
    return sc, {shift: ref.images(sc, 90.0, 90, 70, shift) for shift in (True, False)}


@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
def test_tile_route_against_the_restatement_and_the_exact_route(native, shift):
    """Ten chunks of 32 pulses, and again as one chunk of 320 across the 256-pulse batch boundary; the exact kernel on the same
    pulses through SARX_TDBP_TILE=0."""
    sc, want = native
    res = _pair(sc, 90.0, 90, 70, shift)
    _assert_pair(res, want[shift], "tile")
    one = _pair(sc, 90.0, 90, 70, shift, chunks=1)
    _assert_pair(one, want[shift], "tile")
    with _env("SARX_TDBP_TILE", "0"):
        exact = _pair(sc, 90.0, 90, 70, shift)
    _assert_pair(exact, want[shift], "exact")
    for name, got in (("ten chunks", res), ("one chunk", one)):
        for c, (a, b) in enumerate(((got.img1, exact.img1), (got.img2, exact.img2))):
            err = ref.rel_l2(a, b)
            print(f"tile ({name}) against exact, channel {c}: rel L2 {err:.2e}")
            assert err < KERNEL_TOL
    # the same fp32 terms added in fp64 in another order
    assert max(ref.rel_l2(one.img1, res.img1), ref.rel_l2(one.img2, res.img2)) < 1e-12


def test_more_chunks_asked_for_than_the_union_has_pulses():
    """The stationary scene on 33 x 17 pixels (ragged tiles in both directions), channel 0 on pulses [3, 48) and channel 1 on
    [0, 45): a union of 48 pulses and chunks=64, so the chunk picker stops at one pulse per chunk, 48 chunks, and at either end
    of the union three chunks hold a pulse of one channel only."""
    sc = ref.stationary_scene()
    first, n_used = (3, 0), 45
    want = ref.pair_images(sc["raw"], sc["pos"], sc["vel"], sc["t_vec"], sc["t_start"], sc["num_samples"], 400.0, 33, 17, sc["k"],
                           sc["rx_offsets"], sc["chirp_centre"], first, n_used, rc=sc.get("rc"))   # the compressed pulses, if an earlier test left them
    res = _pair(sc, 400.0, 33, 17, (first, n_used), chunks=64)
    print(f"route {res.route}")
    for c, img in enumerate((res.img1, res.img2)):
        err = ref.rel_l2(img, want[c])
        print(f"channel {c}: rel L2 {err:.2e}")
        assert err < TOL, c


def test_tile_route_with_a_focus_velocity(native):
    sc, _ = native
    vf = (2.0, 6.0, 0.0)
    res = _pair(sc, 90.0, 90, 70, True, vf)
    _assert_pair(res, ref.images(sc, 90.0, 90, 70, True, vf), "tile")


@pytest.mark.parametrize("grid", [(40, 40), (24, 20)], ids=["focus-tile", "focus-exact"])
def test_zero_offsets_reproduce_the_single_channel_focus(grid):
    """Offsets (0, 0), chirp centre 0, no shift, the same spotlight raw as both channels: the two images are the same bits, and
    both are tdbp_gpu's image for a platform at rest (vel_plat = 0: no stop-and-go displacement, no Doppler shift) within 2e-6 -
    on the 40 x 40 grid both take their tile kernels (with no offset the pair's own condition is met trivially), on 24 x 20 the
    exact ones."""
    import sarx
    sc = tb.tdbp_scene(n_pulses=160, seed=2, k=tb.scaled_constants(), swath=400.0)
    nx, ny = grid
    raw = sc["raw"].astype(np.complex64)
    res = sarx.tdbp_pair(raw, raw, sc["pos"], sc["vel"], (0.0, 0.0), sc["t_start"], sc["num_samples"], sc["t_vec"], sc["swath"], nx, ny,
                         chirp_centre=0.0, pulse_shift=False, consts=sc["k"])
    assert res.route == ("tile" if grid == (40, 40) else "exact") and res.lag_s == 0.0
    assert res.img1.tobytes() == res.img2.tobytes()
    one = sarx.tdbp_gpu(raw, sc["pos"], np.zeros_like(sc["vel"]), sc["t_start"], sc["num_samples"], np.zeros(3), sc["t_vec"], sc["swath"],
                        nx, ny, consts=sc["k"])
    err = ref.rel_l2(res.img1, one)
    print(f"pair against tdbp_gpu: rel L2 {err:.2e}")
    assert err < KERNEL_TOL


@pytest.fixture(scope="module")
def mover():
    sc = ref.mover_scene()
    return sc, ref.images(sc, 360.0, 90, 70, True), _pair(sc, 360.0, 90, 70, True)


def test_clutter_cancels_on_the_device(mover):
    """The stationary scene with the shift: |I0 - I1| / |I0| < 2e-4 (two parity bars; the restatement has 1.9e-8).  Every scene:
    the DPCA difference itself agrees with the restatement's to 2e-4 of |I0|."""
    sc = ref.stationary_scene()
    res = _pair(sc, 400.0, 40, 40, True)
    resid = ref.rel_l2(res.img2, res.img1)
    print(f"stationary residue on the device {resid:.3e}")
    assert resid < 2e-4
    cases = [(res, ref.images(sc, 400.0, 40, 40, True)), (_pair(sc, 400.0, 40, 40, False), ref.images(sc, 400.0, 40, 40, False)),
             (mover[2], mover[1])]
    for got, want in cases:
        err = float(np.linalg.norm((got.img1 - got.img2) - (want[0] - want[1])) / np.linalg.norm(want[0]))
        print(f"DPCA difference against the restatement: {err:.3e}")
        assert err < 2e-4


def test_mover_peak_and_ati_phase(mover):
    """The DPCA peak pixel is the restatement's, and the ATI phase there is the restatement's to 2 * 1e-4 * |I0| / |I0[peak]| rad:
    each channel may be off by 1e-4 |I0| in all, at worst all of it on this pixel and at right angles to its value."""
    sc, want, res = mover
    _assert_pair(res, want)
    d_ref, d_gpu = np.abs(want[0] - want[1]), np.abs(res.img1 - res.img2)
    at = np.unravel_index(np.argmax(d_ref), d_ref.shape)
    assert np.unravel_index(np.argmax(d_gpu), d_gpu.shape) == at
    ph_ref = np.angle(want[0][at] * np.conj(want[1][at]))
    ph_gpu = np.angle(res.img1[at] * np.conj(res.img2[at]))
    bound = 2 * 1e-4 * np.linalg.norm(want[0]) / abs(want[0][at])
    print(f"ATI phase {ph_gpu:.6f} against {ph_ref:.6f}, bound {bound:.2e}; v_los {res.v_los(ph_gpu):.3f} m/s")
    assert abs(np.angle(np.exp(1j * (ph_gpu - ph_ref)))) < bound
    assert abs(res.v_los(ph_gpu) - ref.v_los_true(sc, ref.MOVER_AT, ref.MOVER_V)) < 0.04 * ref.v_los_true(sc, ref.MOVER_AT, ref.MOVER_V)


def test_output_forms_reruns_and_device_residency(mover):
    """complex64 = the complex128 sums rounded once; reruns are the same bits; device-resident raw and outputs give the same bits
    as host arrays; the products come out of the complex64 pair."""
    import sarx
    sc, _, res = mover
    ctx = sarx.default_context()
    again = _pair(sc, 360.0, 90, 70, True)
    assert again.img1.tobytes() == res.img1.tobytes() and again.img2.tobytes() == res.img2.tobytes()
    narrow = _pair(sc, 360.0, 90, 70, True, dtype=np.complex64)
    assert narrow.img1.dtype == np.complex64
    assert narrow.img1.tobytes() == res.img1.astype(np.complex64).tobytes() and narrow.img2.tobytes() == res.img2.astype(np.complex64).tobytes()
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    try:
        wide = _pair(sc, 360.0, 90, 70, True, raw=d_raw)
        assert wide.img1.tobytes() == res.img1.tobytes() and wide.img2.tobytes() == res.img2.tobytes()
        dev = _pair(sc, 360.0, 90, 70, True, raw=d_raw, device_output=True)
        try:
            assert dev.img1.shape == (70, 90) and dev.img1.numpy().tobytes() == narrow.img1.tobytes() and dev.img2.numpy().tobytes() == narrow.img2.tobytes()
            prod = dev.ati_dpca()
            np.testing.assert_allclose(prod["dpca_mag"], np.abs(narrow.img1 - narrow.img2), rtol=1e-5, atol=1e-6 * float(np.abs(narrow.img1).max()))
        finally:
            dev.release()
    finally:
        for b in d_raw:
            b.release()


def test_windowed_compression_equals_the_full_one():
    """The sample window is a bound: compressing every sample (SARX_TDBP_FULL_RC=1, read when the plan is made) changes the image
    by no more than another transform length does, < 2e-6."""
    import sarx
    from sarx import tdbp as _tdbp
    sc = ref.stationary_scene()
    k = dict(sc["k"], K_RATE=sc["k"]["K_RATE"] * (1 + 1e-12))              # plans of their own in the cache, windowed ...
    sc_w = dict(sc, k=k)
    res = _pair(sc_w, 400.0, 40, 40, True)
    plan = _tdbp.cached_plan(sarx.default_context(), k, 160, sc["num_samples"], 40, 40)
    lo, hi = plan.last_window()
    assert 0 < lo < hi < sc["num_samples"], (lo, hi)                        # a window was used
    k2 = dict(sc["k"], K_RATE=sc["k"]["K_RATE"] * (1 - 1e-12))             # ... and full (1e-12 of the chirp rate: 1e-10 rad)
    with _env("SARX_TDBP_FULL_RC", "1"):
        full = _pair(dict(sc, k=k2), 400.0, 40, 40, True)
        assert _tdbp.cached_plan(sarx.default_context(), k2, 160, sc["num_samples"], 40, 40).last_window() == (0, sc["num_samples"])
    for a, b in ((res.img1, full.img1), (res.img2, full.img2)):
        err = ref.rel_l2(a, b)
        print(f"windowed against full compression: rel L2 {err:.2e}")
        assert err < KERNEL_TOL


def test_refusals_with_a_live_plan():
    """What needs the plan's pulse count: pulse ranges past the end, a zero vel_tx row; and the route query before any pair call."""
    import ctypes as C
    import sarx
    sc = ref.stationary_scene()
    with pytest.raises(sarx.SarxError, match="outside"):
        _pair(sc, 400.0, 40, 40, ((1, 0), 160))
    vel = sc["vel"].copy()
    vel[77] = 0.0
    with pytest.raises(sarx.SarxError, match="vel_tx row 77"):
        _pair(dict(sc, vel=vel), 400.0, 40, 40, True)
    ctx = sarx.default_context()
    plan = sarx.TdbpPlan(ctx, 16, 256, 8, 8, sc["k"])
    try:
        tile = C.c_int(7)
        assert ctx.lib.sarx_tdbp_pair_route(plan.h, C.byref(tile)) == -1 and tile.value == 7
        assert "pair call" in ctx.last_error()
    finally:
        plan.close()


def test_the_device_pair_feeds_the_gmti_chain():
    """The CSA script's orbit (along track = rows): the complex64 device pair of a mover scene goes into sarx.gmti_detect as it
    is, with range_axis = the slant range of the columns at mid-aperture and cross_range = the y axis; the reports are those of
    tests/_gmti_numpy.py on the same images, under the bars of tests/test_gpu_gmti.py."""
    import sarx
    ctx = sarx.default_context()
    k = tb.scaled_constants()
    stat = [(y, x, rcs) for x, y, rcs in ref.six_scatterers()]
    sc = ref.scene(320, k, stat, [(0.0, 495.0, 50.0, (10.0, 0.0, 0.0))], orbit="csa")
    nx, ny = 90, 70
    d_raw = [ctx.to_device(r) for r in sc["raw"]]
    dev = _pair(sc, 360.0, nx, ny, True, raw=d_raw, device_output=True)
    try:
        xs, ys = np.linspace(-180.0, 180.0, nx), np.linspace(-180.0, 180.0, ny)
        p_mid = sc["pos"][len(sc["t_vec"]) // 2]
        ra = np.sqrt((xs - p_mid[0]) ** 2 + p_mid[1] ** 2 + p_mid[2] ** 2)
        lam = k["C"] / k["FC"]
        guard, train, pfa = (2, 2), (8, 8), 1e-3
        rep = sarx.gmti_detect(dev.img1, dev.img2, ra, ys, wavelength_m=lam, platform_speed_mps=sc["speed"], lag_s=dev.lag_s, guard=guard,
                               train=train, pfa=pfa, max_detections=4096)
        s1, s2 = dev.img1.numpy(), dev.img2.numpy()
        m = dev.ati_dpca()["dpca_mag"]
        o = gref.cfar(m, guard, train, pfa=pfa)
        d = rep.detections
        cells = list(zip(d["i"].tolist(), d["j"].tolist()))
        missing, extra = gref.compare(cells, o)
        assert not missing and not extra, (missing[:10], extra[:10], len(cells), len(o["cells"]))
        assert len(cells) >= 1
        ii, jj = d["i"], d["j"]
        np.testing.assert_array_equal(d["power"], o["power"][ii, jj])
        np.testing.assert_allclose(d["mean"], o["mean"][ii, jj], rtol=1e-6)
        want = gref.interferogram(s1, s2, cells, 0.0)
        scale = np.array([np.sum(np.abs(s1[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]) * np.abs(s2[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]))
                          for i, j in cells])
        assert np.all(np.abs(d["interf"] - want) <= 1e-6 * scale)
        np.testing.assert_array_equal(d["range_m"], ra[jj])
        np.testing.assert_array_equal(d["cross_range_m"], ys[ii])
        np.testing.assert_allclose(d["v_los_mps"], -lam * np.angle(want) / (4 * np.pi * dev.lag_s), atol=1e-4)
        assert rep.v_ambiguity_mps == pytest.approx(dev.v_ambiguity)
        # the strongest DPCA cell is reported, and its radial speed is the mover's within the CPU test's 4 %
        pi, pj = np.unravel_index(np.argmax(m), m.shape)
        assert (int(pi), int(pj)) in cells
        r = d[(d["i"] == pi) & (d["j"] == pj)][0]
        truth = ref.v_los_true(sc, (0.0, 495.0), (10.0, 0.0, 0.0))
        print(f"{len(cells)} reports; strongest at ({ys[pi]:.1f}, {xs[pj]:.1f}) m, v_los {r['v_los_mps']:.3f} against {truth:.3f} m/s")
        assert abs(r["v_los_mps"] - truth) < 0.04 * truth
    finally:
        dev.release()
        for b in d_raw:
            b.release()
