"""The back-projection kernels (focus, focus-velocity search, two-receiver pair; csrc/tdbp_pixel.hpp) against the oracle PIXEL BY PIXEL
on noise pulses: pixel_err = max |gpu - oracle| / rms(|oracle|) < tol(case), on the cases of tests/_tdbp_noise.py.

The other back-projection tests hold relative L2 over the whole image below 1e-4 on scenes of a few point targets, whose energy sits
in a few dozen pixels; the ragged tiles, the ends of the sample window, the zero padding of the interpolation and a pulse lost at a
batch or chunk boundary of one tile are outside their sight (tests/test_tdbp_pixelwise.py has the figures).  Here every sample
matters to the pixels that read it and every pixel is compared.

Cases (33 x 17 pixels = 3 x 2 tiles with a one-pixel ragged column and row, 288 pulses, vel_focus (3, -2, 0)):
  N1       batch_constants(): 22004 samples, 12000 taps, 33 m scene: the tile route by geometry
  N2       scaled_constants(): 1122 samples, 400 m scene: the exact route by geometry
  E-lo/hi  N1 / N2 with t_start moved until the two outermost image rows read off that end of the pulse: every branch of the zero
           padding of tdbp_sample runs, the outermost row is exactly zero, the sample window is clamped
  G1       N2 on 17 x 1 and 1 x 17 pixels: too thin for a tile reach

tol(case) = 3 x max(coordinate floor, compression floor), both measured on the oracle when the test runs (_tdbp_noise.pixel_floor),
capped by 1 / (8 sqrt(n_pulses)) = 7.4e-3.  The coordinate floor is the oracle against itself with t_start moved by 1e-6 sample (the
coordinate error csrc/tdbp_pixel.hpp documents for the tile form: float32 roundings of the coordinate that flip), the compression
floor the oracle on compressed pulses carrying the 1e-5 relative L2 that test_range_compression_matches_oracle allows.

Measured: floors on the CPU, device figures on an MI355X (worst pixel, and the whole-image relative L2 of the same image beside it):

  case                       coord floor  rc floor   tol       device pixel_err    device rel L2
  N1 focus, tile / exact     4.2e-4       2.1e-5     1.3e-3    3.5e-6 / 3.5e-6     1.7e-6
  N1 focus over stale rc     4.2e-4       2.1e-5     1.3e-3    3.5e-6              1.7e-6
  N2 focus                   3.8e-5       2.2e-5     1.1e-4    3.4e-6              8.6e-7
  N1-lo / N1-hi focus        2.0e-4 / 5.0e-4  2.4e-5 5.9e-4 / 1.5e-3  4.9e-6 / 4.3e-6  1.7e-6 / 1.8e-6
  N2-lo / N2-hi focus        3.2e-5 / 6.8e-5  3.4e-5 1.0e-4 / 2.0e-4  2.3e-6 / 2.4e-6  7.6e-7 / 7.9e-7
  G1-row / G1-col focus      1.8e-5 / 2.3e-5  1.3e-5 5.4e-5 / 7.0e-5  1.7e-6 / 2.2e-6  6.4e-7 / 8.8e-7
  N1 search, 3 hypotheses    2.9e-4 .. 4.2e-4        8.7e-4 .. 1.3e-3  3.5e-6 .. 4.7e-6  1.7e-6   (nine chunks and one: the same)
  N2 / N2-lo search          3.7e-5 / 3.4e-5         1.1e-4 / 1.0e-4   3.4e-6 / 2.4e-6   8.7e-7 / 7.6e-7
  N1 pair (24 m), all routes 6.0e-4       2.4e-5     1.8e-3    3.2e-6 .. 4.0e-6    1.6e-6 .. 1.8e-6
  N1w pair (33 m, exact)     4.8e-4       2.4e-5     1.5e-3    4.2e-6              1.7e-6
  N2 / N2-hi pair            5.1e-5 / 6.3e-5  2.7e-5 1.5e-4 / 1.9e-4  2.8e-6 / 2.4e-6  7.5e-7 / 7.9e-7
  tile against exact, N1     bar = coord floor alone: focus 1.5e-7 against 4.2e-4, pair 2.8e-7 against 6.0e-4

The device stands two orders of magnitude under its tolerance everywhere: it rounds the float32 coordinate as the oracle does on all
but a handful of the 1.6e5 (pulse, pixel) pairs, so what is left is the single-precision compression and interpolation.  The tolerance
is nevertheless the measured floor and not the device's figure: it is what the documented arithmetic is entitled to.
"""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

from oracle.csa_oracle import rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_noise as tn  # noqa: E402
import _tdbp_search_numpy as sref  # noqa: E402

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _exact_kernel():
    """SARX_TDBP_TILE=0: the switch the shared tile condition reads at every call."""
    old = os.environ.get("SARX_TDBP_TILE")
    os.environ["SARX_TDBP_TILE"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["SARX_TDBP_TILE"]
        else:
            os.environ["SARX_TDBP_TILE"] = old


@functools.lru_cache(maxsize=None)
def _oracle(name, kind="focus", shift=False):
    """The oracle's images of a case, computed once for the module and left unchanged."""
    img = tn.oracle_images(tn.case(name, kind), shift)
    img.setflags(write=False)
    return img


def _check(label, got, want, tol):
    """Every image of got against want, per pixel; where the oracle is exactly zero (every tap in the padding) so is the device."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.complex128 and got.shape == want.shape
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        err = tn.pixel_err(g, w)
        print(f"{label} image {i}: pixel_err {err:.2e} tol {tol:.2e} (whole-image rel L2 {rel_l2(g, w):.2e})")
        worst = max(worst, err)
    assert worst < tol, label
    assert not np.any(got[want == 0]), label


def _plan(c):
    import sarx
    return sarx.TdbpPlan(sarx.default_context(), c["n_pulses"], c["num_samples"], c["nx"], c["ny"], c["k"])


def _focus(plan, c, raw=None, **kw):
    return plan.focus(tn.raw_of(c) if raw is None else raw, c["pos"], c["vel"], c["t_start"], c["vel_focus"], c["t_vec"], c["swath"], **kw)


# ---- focus -----------------------------------------------------------------------------------------------------------------------

def test_focus_native_tile_and_exact_kernel():
    """N1 through the tile kernel (by geometry) and the exact kernel (by the switch): either against the oracle, and against each
    other under the coordinate floor alone - the expansions' 1e-9 m are 4e-7 rad, the fp32 t_shift < 1e-6 sample."""
    c = tn.case("N1")
    f = tn.pixel_floor(c)
    plan = _plan(c)
    tile = _focus(plan, c)
    lo, hi = plan.last_window()
    with _exact_kernel():
        exact = _focus(plan, c)
    plan.close()
    assert 0 < lo < hi < c["num_samples"]
    assert not np.array_equal(tile, exact)                            # two different kernels ran
    _check("N1 tile", tile[None], _oracle("N1"), f["tol"])
    _check("N1 exact", exact[None], _oracle("N1"), f["tol"])
    err = tn.pixel_err(tile, exact)
    print(f"N1 tile against exact: pixel_err {err:.2e} coordinate floor {f['coord']:.2e}")
    assert err < f["coord"]


def test_focus_scaled_exact_kernel_by_geometry():
    """N2: 12.5 x 25 m pixels are beyond the tile expansion, so the switch changes nothing - the same kernel, the same bits."""
    c = tn.case("N2")
    plan = _plan(c)
    img = _focus(plan, c)
    with _exact_kernel():
        forced = _focus(plan, c)
    plan.close()
    assert np.array_equal(img, forced)
    _check("N2 exact", img[None], _oracle("N2"), tn.pixel_floor(c)["tol"])


@pytest.mark.parametrize("name", ["N1-lo", "N1-hi", "N2-lo", "N2-hi"])
def test_focus_reads_off_the_end_of_the_pulse(name):
    c = tn.case(name)
    plan = _plan(c)
    img = _focus(plan, c)
    lo, hi = plan.last_window()
    plan.close()
    print(f"{name}: window [{lo}, {hi}) of {c['num_samples']}")
    if name.endswith("lo"):
        assert lo == 0 and 0 < hi < c["num_samples"]
    else:
        assert hi == c["num_samples"] and 0 < lo < hi
    want = _oracle(name)
    assert not np.any(want[0, 0 if name.endswith("lo") else -1])      # the outermost row reads padding only
    _check(name, img[None], want, tn.pixel_floor(c)["tol"])


@pytest.mark.parametrize("name", ["G1-row", "G1-col"])
def test_focus_grids_one_pixel_thin(name):
    c = tn.case(name)
    plan = _plan(c)
    img = _focus(plan, c)
    plan.close()
    _check(name, img[None], _oracle(name), tn.pixel_floor(c)["tol"])


def test_focus_window_over_stale_samples():
    """One plan: 1000 x another realisation compressed in full (want_rc), then the windowed focus of the case's pulses.  A read
    outside [lo, hi) now costs a thousand samples instead of one."""
    c = tn.case("N1")
    plan = _plan(c)
    _, rc = _focus(plan, c, raw=tn.stale_pulses(c), want_rc=True)
    assert plan.last_window() == (0, c["num_samples"])
    img = _focus(plan, c)
    lo, hi = plan.last_window()
    plan.close()
    assert 0 < lo < hi < c["num_samples"]
    own = np.sqrt(np.mean(np.abs(tn.rc_of(c)) ** 2))
    assert np.sqrt(np.mean(np.abs(rc[:, :lo]) ** 2)) > 500 * own and np.sqrt(np.mean(np.abs(rc[:, hi:]) ** 2)) > 500 * own
    _check("N1 over stale samples", img[None], _oracle("N1"), tn.pixel_floor(c)["tol"])


# ---- search ----------------------------------------------------------------------------------------------------------------------

def _search(c, **kw):
    import sarx
    return sarx.tdbp_search(tn.raw_of(c), c["pos"], c["vel"], c["t_start"], c["num_samples"], tn.search_hyps(c), c["t_vec"], c["swath"],
                            c["nx"], c["ny"], images=True, consts=c["k"], **kw)


@functools.lru_cache(maxsize=None)
def _search_oracle(name):
    c = tn.case(name)
    hyps = tn.search_hyps(c)
    want = sref.stack_images(tn.search_scene(c), hyps, c["nx"], c["ny"], rc=tn.rc_of(c))
    want.setflags(write=False)
    return want, [tn.pixel_floor(tn.with_focus(c, v))["tol"] for v in hyps]


def _check_stack(label, res, name):
    want, tols = _search_oracle(name)
    assert res.images.shape == want.shape
    for h in range(len(tols)):
        _check(f"{label} hypothesis {h}", res.images[h][None], want[h][None], tols[h])


def test_search_native_tile_route():
    """Nine chunks of 32 pulses by default; chunks=1 puts the 256-pulse batch boundary inside the chunk."""
    c = tn.case("N1")
    res = _search(c)
    assert res.route == "tile"
    _check_stack("N1 search", res, "N1")
    one = _search(c, chunks=1)
    assert one.route == "tile"
    _check_stack("N1 search, one chunk", one, "N1")


def test_search_scaled_exact_route():
    c = tn.case("N2")
    res = _search(c)
    assert res.route == "exact"
    _check_stack("N2 search", res, "N2")


def test_search_reads_off_the_low_end():
    c = tn.case("N2-lo")
    res = _search(c)
    assert res.route == "exact"
    _check_stack("N2-lo search", res, "N2-lo")


# ---- pair ------------------------------------------------------------------------------------------------------------------------

def _pair(c, shift, **kw):
    import sarx
    raw = tn.raw_of(c)
    res = sarx.tdbp_pair(raw[0], raw[1], c["pos"], c["vel"], c["rx_offsets"], c["t_start"], c["num_samples"], c["t_vec"], c["swath"],
                         c["nx"], c["ny"], vel_focus=c["vel_focus"], chirp_centre=c["chirp_centre"], pulse_shift=shift, consts=c["k"], **kw)
    return res.route, np.stack((res.img1, res.img2))


@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
def test_pair_native_tile_and_exact_kernel(shift):
    """The pair's N1 is 24 m wide: at the focus's 33 m the pair's own tile bound refuses (_tdbp_noise.PAIR_SWATH).  Nine chunks of 32
    pulses, one chunk across the 256-pulse batch boundary, and the exact kernel by the switch."""
    c = tn.case("N1", "pair")
    f = tn.pixel_floor(c, shift)
    want = _oracle("N1", "pair", shift)
    route, tile = _pair(c, shift)
    assert route == "tile"
    _check("N1 pair tile", tile, want, f["tol"])
    route, one = _pair(c, shift, chunks=1)
    assert route == "tile"
    _check("N1 pair tile, one chunk", one, want, f["tol"])
    with _exact_kernel():
        route, exact = _pair(c, shift)
    assert route == "exact"
    _check("N1 pair exact", exact, want, f["tol"])
    for ch in range(2):
        err = tn.pixel_err(tile[ch], exact[ch])
        print(f"N1 pair tile against exact, channel {ch}: pixel_err {err:.2e} coordinate floor {f['coord']:.2e}")
        assert err < f["coord"]


def test_pair_native_at_the_focus_scene_size():
    """N1w: the 33 m of the focus's N1, where |q|^2 |off| / (sqrt(3) d^2) = 1.2e-9 m is over the pair's 1e-9 m bound: the exact kernel by
    geometry, on native pulses."""
    c = tn.case("N1w", "pair")
    route, img = _pair(c, True)
    assert route == "exact"
    _check("N1w pair", img, _oracle("N1w", "pair", True), tn.pixel_floor(c, True)["tol"])


@pytest.mark.parametrize("shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("name", ["N2", "N2-hi"])
def test_pair_scaled_exact_kernel(name, shift):
    c = tn.case(name, "pair")
    with _exact_kernel():
        route, img = _pair(c, shift)
    assert route == "exact"
    _check(f"{name} pair", img, _oracle(name, "pair", shift), tn.pixel_floor(c, shift)["tol"])
