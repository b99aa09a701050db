"""CPU checks of the two-receiver back-projection (include/sarx_tdbp_pair.h, csrc/tdbp_pair.hip, sarx/tdbp_pair.py): header,
binding and exported symbols, every refusal that needs no device, the sanitizer driver, and the physics of the NumPy restatement
(tests/_tdbp_pair_numpy.py, which also fixes the scenes of tests/test_gpu_tdbp_pair.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_pair_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_tdbp_pair.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")
NAMES = ("sarx_tdbp_pair_check", "sarx_tdbp_pair_dev", "sarx_tdbp_pair_host", "sarx_tdbp_pair_route")
INVALID = -1


def _symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from sarx import _ffi
    syms = _symbols()
    assert syms == sorted(_ffi.TDBP_PAIR_SIGNATURES) == sorted(NAMES)
    assert not set(syms) & set(_ffi.SIGNATURES)                       # sarx.h got no new function
    assert "tdbp_pair" not in open(os.path.join(ROOT, "include", "sarx.h")).read()
    assert C.sizeof(_ffi.TdbpPairParams) == 40
    assert [(_ffi.TdbpPairParams.rx_offset_m.offset, _ffi.TdbpPairParams.chirp_centre_s.offset, _ffi.TdbpPairParams.first_pulse.offset,
             _ffi.TdbpPairParams.n_used.offset, _ffi.TdbpPairParams.reserved.offset)] == [(0, 16, 24, 32, 36)]


def test_header_is_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "sarx_tdbp_pair.h"\nint main(void) { return sizeof(sarx_tdbp_pair_params) == 40 && '
                   'offsetof(sarx_tdbp_pair_params, first_pulse) == 24 && offsetof(sarx_tdbp_pair_params, n_used) == 32 ? 0 : 1; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_library_exports_the_symbols_and_the_package_the_names():
    import sarx
    from sarx import _ffi
    lib = _ffi.load()
    for s in NAMES:
        assert hasattr(lib, s), s
    for name in ("tdbp_pair", "TdbpPairResult"):
        assert name in sarx.__all__ and hasattr(sarx, name)
    assert lib.sarx_version() >= 100


def _params(off=(-1.5, 1.5), cc=1e-6, first=(1, 0), n_used=7):
    from sarx import _ffi
    return _ffi.TdbpPairParams((C.c_double * 2)(*off), cc, (C.c_int32 * 2)(*first), n_used, 0)


def _refused(rc, word):
    from sarx import _ffi
    msg = _ffi.load().sarx_last_error(None).decode()
    assert rc == INVALID and word in msg, (rc, msg)


def test_params_check_without_a_device():
    from sarx import _ffi
    lib = _ffi.load()
    assert lib.sarx_tdbp_pair_check(8, C.byref(_params())) == 0
    assert lib.sarx_tdbp_pair_check(8, C.byref(_params(first=(0, 0), n_used=8))) == 0
    _refused(lib.sarx_tdbp_pair_check(8, None), "NULL")
    _refused(lib.sarx_tdbp_pair_check(0, C.byref(_params())), "n_pulses")
    for bad in (float("nan"), float("inf"), -float("inf")):
        _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(off=(bad, 1.5)))), "rx_offset_m")
        _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(off=(-1.5, bad)))), "rx_offset_m")
        _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(cc=bad))), "chirp_centre_s")
    for n in (0, -1):
        _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(n_used=n))), "n_used")
    _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(first=(-1, 0)))), "first_pulse")
    _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(first=(0, -1)))), "first_pulse")
    _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(n_used=8))), "outside")            # 1 + 8 > 8
    _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(first=(0, 2), n_used=7))), "outside")
    _refused(lib.sarx_tdbp_pair_check(8, C.byref(_params(first=(2 ** 31 - 1, 0), n_used=2 ** 31 - 1))), "outside")   # no int overflow


@pytest.mark.parametrize("entry", ["sarx_tdbp_pair_dev", "sarx_tdbp_pair_host"])
def test_entry_points_refuse_without_a_device(entry):
    """NULL pointers, both outputs NULL, misaligned outputs, non-finite numbers, a bad scene size and bad pulse ranges are refused
    before the plan is looked at; then a NULL plan and one the library never made."""
    from sarx import _ffi
    f = getattr(_ffi.load(), entry)
    raw = np.zeros(64, np.complex64)
    img = np.zeros(256, np.complex128)
    assert img.ctypes.data % 16 == 0
    pos, vel, tp, vf = np.ones((2, 3)), np.ones((2, 3)), np.arange(2.0), np.zeros(3)
    stale = (C.c_char * 8)()
    for plan in (None, C.addressof(stale)):
        good = dict(raw0=raw.ctypes.data, raw1=raw.ctypes.data, pos=pos.ctypes.data, vel=vel.ctypes.data, tp=tp.ctypes.data, t_start=0.0,
                    vf=vf.ctypes.data, scene=10.0, prm=C.byref(_params(n_used=1)), o128=img.ctypes.data, o64=img.ctypes.data)

        def call(**kw):
            a = dict(good, **kw)
            return f(plan, a["raw0"], a["raw1"], a["pos"], a["vel"], a["tp"], a["t_start"], a["vf"], a["scene"], a["prm"], a["o128"], a["o64"])

        for name in ("raw0", "raw1", "pos", "vel", "tp", "vf", "prm"):
            _refused(call(**{name: None}), "NULL")
        _refused(call(o128=None, o64=None), "both outputs")
        _refused(call(o128=img.ctypes.data + 8), "misaligned")
        _refused(call(o64=img.ctypes.data + 4), "misaligned")
        for bad in (float("nan"), float("inf")):
            v = np.array([0.0, bad, 0.0])
            _refused(call(vf=v.ctypes.data), "vel_focus")
            _refused(call(prm=C.byref(_params(off=(bad, 0.0), n_used=1))), "rx_offset_m")
            _refused(call(prm=C.byref(_params(cc=bad, n_used=1))), "chirp_centre_s")
            _refused(call(scene=bad), "scene_size")
        for bad in (0.0, -3.0):
            _refused(call(scene=bad), "scene_size")
        _refused(call(prm=C.byref(_params(n_used=0))), "n_used")
        _refused(call(prm=C.byref(_params(first=(0, -2), n_used=1))), "first_pulse")
        _refused(call(), "plan")
        _refused(call(o128=None), "plan")
    tile = C.c_int(7)
    for plan in (None, C.addressof(stale)):
        _refused(_ffi.load().sarx_tdbp_pair_route(plan, None), "NULL")
        _refused(_ffi.load().sarx_tdbp_pair_route(plan, C.byref(tile)), "plan")
    assert tile.value == 7


def test_python_wrapper_checks_its_arguments_before_any_device_work():
    import sarx
    from sarx.tdbp_pair import pair_params
    p = pair_params(10, (-1.0, 1.0), 2e-6, True)
    assert (p.first_pulse[0], p.first_pulse[1], p.n_used) == (1, 0, 9)
    p = pair_params(10, (-1.0, 1.0), 2e-6, False)
    assert (p.first_pulse[0], p.first_pulse[1], p.n_used) == (0, 0, 10)
    p = pair_params(10, (-1.0, 1.0), 2e-6, ((2, 3), 4))
    assert (p.first_pulse[0], p.first_pulse[1], p.n_used) == (2, 3, 4)
    with pytest.raises(ValueError):
        pair_params(10, (1.0, 2.0, 3.0), 0.0, True)
    r = sarx.TdbpPairResult(None, None, 2e-4, 0.03, "exact", None)
    assert r.v_ambiguity == pytest.approx(0.03 / (4 * 2e-4))
    assert r.v_los(-0.5) == pytest.approx(0.03 * 0.5 / (4 * np.pi * 2e-4))
    assert np.allclose(r.v_los(np.array([0.0, np.pi])), [0.0, -r.v_ambiguity])


def test_tdbp_pair_entry_points_under_address_and_ub_sanitizer():
    """The stand-alone driver (its own main, against libsarx_asan.so), built and run on the CPU."""
    r = subprocess.run(["make", "-j8", "asan-tdbppair"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "tdbppair_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_driver_names_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "tdbppair_asan_test.cpp")).read()
    code = re.sub(r"//[^\n]*", "", drv)                               # a name in a comment does not count
    missing = [n for n in _symbols() if not re.search(r"\b" + n + r"\b", code)]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------------
# the restatement's physics: what the feature is for
# ---------------------------------------------------------------------------------------------------------------------
def test_clutter_cancels_under_the_pulse_shift_and_not_without_it():
    """Six stationary scatterers, 160 pulses, 40 x 40 over 400 m, receivers at -+ V / PRF.  Measured: with the DPCA pulse shift
    |I0 - I1| / |I0| = 1.9e-8 (the phase centres coincide; what is left is the complex64 cast of the echoes and fp64 rounding of
    a 3e7-revolution phase), without it 3.2e-2 (geometric: the two apertures are displaced by one pulse).  Bars: 1e-6 for the
    shifted residue - fifty times the measured value, and still a thousand times below the parity bar the GPU test holds the
    images to, so a one-pulse or one-sample slip (1e-2 and up) cannot hide; the unshifted residue at least 1e4 times the
    shifted one (measured 1.6e6: 'much greater' with two orders of margin) and between 1e-2 and 1e-1."""
    sc = ref.stationary_scene()
    a = ref.images(sc, 400.0, 40, 40, True)
    b = ref.images(sc, 400.0, 40, 40, False)
    shifted, unshifted = ref.rel_l2(a[1], a[0]), ref.rel_l2(b[1], b[0])
    print(f"shifted residue {shifted:.3e}, unshifted {unshifted:.3e}")
    assert shifted < 1e-6
    assert unshifted > 1e4 * shifted and 1e-2 < unshifted < 1e-1


def test_ati_phase_of_the_dpca_peak_gives_the_radial_speed():
    """The same scatterers and a mover at (495, 0) m with velocity (0, 10, 0) m/s, 320 pulses, 90 x 70 over 360 m.  Measured: the
    DPCA peak lies at (2.0, 7.8) m (the radial speed shifts the mover 493 m along track) and stands 1092 x above the median; its
    ATI phase -0.594 rad gives v_los = 7.34 m/s against the true 7.46 (1.5 %).  Bars: the peak at least 100 x the median (a
    tenth of the measured ratio: the clutter floor depends on the scatterers drawn); v_los within 4 % of the truth - the pixel
    grid puts the sample up to half a pixel (2.0 x 2.6 m of a response 4 m wide in range) off the response's centre, where the
    phase of the half-band compressed pulse has moved; the measured error is 1.5 %, and a wrong lag (one pulse: 100 %), sign
    (200 %) or wavelength could not pass."""
    sc = ref.mover_scene()
    img = ref.images(sc, 360.0, 90, 70, True)
    d = np.abs(img[0] - img[1])
    iy, ix = np.unravel_index(np.argmax(d), d.shape)
    xs, ys = np.linspace(-180, 180, 90), np.linspace(-180, 180, 70)
    lam = sc["k"]["C"] / sc["k"]["FC"]
    phase = float(np.angle(img[0, iy, ix] * np.conj(img[1, iy, ix])))
    v = -lam * phase / (4 * np.pi * sc["lag"])
    truth = ref.v_los_true(sc, ref.MOVER_AT, ref.MOVER_V)
    print(f"peak ({xs[ix]:.1f}, {ys[iy]:.1f}) m, {d.max() / np.median(d):.0f} x median, phase {phase:.4f} rad, v_los {v:.3f} vs {truth:.3f} m/s")
    assert sc["lag"] == pytest.approx(1.0 / sc["k"]["PRF"], rel=1e-12)
    assert d.max() > 100 * np.median(d)
    assert abs(xs[ix]) < 20 and abs(ys[iy]) < 20
    assert abs(v - truth) < 0.04 * truth
    assert lam / (4 * sc["lag"]) > 2 * truth                                                # inside the unambiguous span


def test_focus_velocity_of_the_mover_puts_it_at_its_true_position():
    """A mover at (40, -30) m with velocity (0, 10, 0) m/s among the scatterers, 320 pulses, 40 x 40 over 400 m.  Measured: with
    vel_focus = its velocity the strongest pixel of channel 0 is (35.9, -25.6) m, the grid point next to the truth, 3.7 x the
    peak of vel_focus = 0 (which lies at (25.6, -25.6) m), and the ATI phase there is -0.001 rad: focused with its own
    velocity the mover looks stationary.  Bars: within one pixel (10.26 m) of the true position on both axes;
    |ATI phase| < 0.02 rad (half of the 0.04 rad that 0.5 m/s of unmatched radial speed gives; measured 0.001)."""
    sc = ref.focus_scene()
    img = ref.images(sc, 400.0, 40, 40, True, ref.MOVER_V)
    still = ref.images(sc, 400.0, 40, 40, True)
    a = np.abs(img[0])
    iy, ix = np.unravel_index(np.argmax(a), a.shape)
    ax = np.linspace(-200, 200, 40)
    phase = float(np.angle(img[0, iy, ix] * np.conj(img[1, iy, ix])))
    print(f"peak ({ax[ix]:.1f}, {ax[iy]:.1f}) m, {a.max() / np.abs(still[0]).max():.2f} x the vel_focus = 0 peak, ATI phase {phase:.5f} rad")
    pixel = ax[1] - ax[0]
    assert abs(ax[ix] - ref.FOCUS_AT[0]) <= pixel and abs(ax[iy] - ref.FOCUS_AT[1]) <= pixel
    assert a.max() > np.abs(still[0]).max()
    assert abs(phase) < 0.02
