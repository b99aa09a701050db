"""CPU checks of the ground relocation of GMTI reports (include/sarx_relocate.h, csrc/relocate.hip, sarx/relocate.py): header,
binding and exported symbols, every refusal that needs no device, the sanitizer driver, and the geometry and physics of the NumPy
restatement (tests/_relocate_numpy.py, which tests/test_gpu_relocate.py holds the kernels to)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _relocate_numpy as ref  # noqa: E402
import _tdbp_multi_numpy as mref  # noqa: E402
from oracle import tdbp_oracle as tb  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_relocate.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")
NAMES = ("sarx_relocate_check", "sarx_relocate_dev")
INVALID = -1


def _symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


# ---------------------------------------------------------------------------------------------------------------------
# header and binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    import sarx
    from sarx import _ffi
    from sarx.relocate import RECORD_DTYPE
    syms = _symbols()
    assert syms == sorted(_ffi.RELOCATE_SIGNATURES) == sorted(NAMES)
    assert not set(syms) & set(_ffi.SIGNATURES)                       # sarx.h got no new function
    assert "relocate" not in open(os.path.join(ROOT, "include", "sarx.h")).read()
    P, R = _ffi.RelocateParams, _ffi.RelocateRecord
    assert (C.sizeof(P), C.sizeof(R)) == (128, 64)
    assert [getattr(P, n).offset for n, _ in P._fields_] == [0, 24, 48, 56, 64, 72, 80, 88, 96, 104, 112, 116, 120, 124]
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    assert [n for n, _ in R._fields_] == list(RECORD_DTYPE.names) == list(ref.RECORD_DTYPE.names)
    assert [RECORD_DTYPE.fields[n][1] for n in RECORD_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60] and RECORD_DTYPE == ref.RECORD_DTYPE
    assert (_ffi.RELOCATE_OK, _ffi.RELOCATE_NO_SPEED, _ffi.RELOCATE_NO_SOLUTION, _ffi.RELOCATE_OFF_GRID, _ffi.RELOCATE_OVERFLOW) == \
        (ref.OK, ref.NO_SPEED, ref.NO_SOLUTION, ref.OFF_GRID, ref.OVERFLOW) == (0, 1, 2, 3, 4)
    lib = _ffi.load()
    assert lib.sarx_version() == 206
    for s in NAMES:
        assert hasattr(lib, s), s
    for name in ("ground_relocate", "reference_geometry", "relocate_frames", "RelocateResult"):
        assert name in sarx.__all__ and hasattr(sarx, name)


def test_header_is_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "sarx_relocate.h"\nint main(void) { return sizeof(sarx_relocate_params) == 128 && '
                   'sizeof(sarx_relocate_record) == 64 && offsetof(sarx_relocate_params, vel_ref) == 24 && '
                   'offsetof(sarx_relocate_params, in_dx) == 64 && offsetof(sarx_relocate_params, out_x0) == 80 && '
                   'offsetof(sarx_relocate_params, out_nx) == 112 && offsetof(sarx_relocate_params, reserved) == 124 && '
                   'offsetof(sarx_relocate_record, vx) == 32 && offsetof(sarx_relocate_record, rank) == 48 && '
                   'offsetof(sarx_relocate_record, status) == 52 && offsetof(sarx_relocate_record, flags) == 56 ? 0 : 1; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    from sarx import _ffi
    v = dict(pos_ref=(0.0, -4000.0, 3000.0), vel_ref=(100.0, 0.0, 0.0), in_x0=-180.0, in_y0=-180.0, in_dx=4.0, in_dy=5.0, out_x0=-1000.0,
             out_y0=-1000.0, out_dx=2.0, out_dy=2.0, out_nx=1000, out_ny=1000, max_detections=8, reserved=0)
    v.update(kw)
    return _ffi.RelocateParams((C.c_double * 3)(*v.pop("pos_ref")), (C.c_double * 3)(*v.pop("vel_ref")), *v.values())


def _refused(rc, word):
    from sarx import _ffi
    msg = _ffi.load().sarx_last_error(None).decode()
    assert rc == INVALID and word in msg, (rc, msg, word)


def test_every_refusal_of_the_parameter_check():
    from sarx import _ffi
    lib = _ffi.load()
    chk = lib.sarx_relocate_check
    assert chk(C.byref(_params())) == 0
    assert chk(C.byref(_params(out_nx=1 << 20, out_ny=1,
                               max_detections=_ffi.TDBP_MULTI_MAX_DETECTIONS, in_dx=-1e-300, out_dy=-2.0, vel_ref=(0.0, 0.0, 0.0)))) == 0
    _refused(chk(None), "NULL")
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(3):
            v = [0.0, -4000.0, 3000.0]
            v[k] = bad
            _refused(chk(C.byref(_params(pos_ref=v))), f"pos_ref[{k}]")
            v = [100.0, 0.0, 0.0]
            v[k] = bad
            _refused(chk(C.byref(_params(vel_ref=v))), f"vel_ref[{k}]")
        for name in ("in_x0", "in_y0", "in_dx", "in_dy", "out_x0", "out_y0", "out_dx", "out_dy"):
            _refused(chk(C.byref(_params(**{name: bad}))), name)
    for name in ("in_dx", "in_dy", "out_dx", "out_dy"):
        for zero in (0.0, -0.0):
            _refused(chk(C.byref(_params(**{name: zero}))), name)
    for name in ("out_nx", "out_ny"):
        for n in (0, -1, (1 << 20) + 1, 2 ** 31 - 1):
            _refused(chk(C.byref(_params(**{name: n}))), name)
    for md in (0, -1, _ffi.TDBP_MULTI_MAX_DETECTIONS + 1, 2 ** 31 - 1):
        _refused(chk(C.byref(_params(max_detections=md))), "max_detections")
    for r in (1, -1):
        _refused(chk(C.byref(_params(reserved=r))), "reserved")
    # without a context the device entry point refuses before it reads anything
    _refused(lib.sarx_relocate_dev(None, C.byref(_params()), None, None, 8, None, 4, None, 8, None, None), "ctx")


def test_python_wrapper_checks_its_arguments_before_any_device_work():
    import sarx
    from sarx.relocate import grid_of, relocate_params
    assert grid_of((360.0, 90, 70)) == (-180.0, -180.0, 360.0 / 89, 360.0 / 69, 90, 70)
    assert grid_of((360.0, 90, 70))[:4] == ref.tdbp_grid(360.0, 90, 70)
    p = relocate_params((1, 2, 3), (4, 5, 6), (360.0, 90, 70), None, 16)
    assert (list(p.pos_ref), list(p.vel_ref), p.in_dx, p.out_dx, p.out_nx, p.out_ny, p.max_detections) == \
        ([1, 2, 3], [4, 5, 6], 360.0 / 89, 360.0 / 89, 90, 70, 16)
    p = relocate_params((1, 2, 3), (4, 5, 6), (360.0, 90, 70), (-500.0, -400.0, 2.0, 3.0, 512, 256), 16)
    assert (p.in_x0, p.out_x0, p.out_y0, p.out_dx, p.out_dy, p.out_nx, p.out_ny) == (-180.0, -500.0, -400.0, 2.0, 3.0, 512, 256)
    for bad in (dict(pos_ref=(1, 2)), dict(vel_ref=(1, 2, 3, 4)), dict(grid=(360.0, 0, 70)), dict(out_grid=(0.0, 0.0, 1.0, 1.0, 4))):
        kw = dict(pos_ref=(1, 2, 3), vel_ref=(4, 5, 6), grid=(360.0, 90, 70), out_grid=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            relocate_params(kw["pos_ref"], kw["vel_ref"], kw["grid"], kw["out_grid"], 16)
    # the reference geometry: linear interpolation at mean(t_pulses), the pair's mean phase centre (off_a + off_b) / 4 ahead
    pos = np.array([[0.0, 0.0, 3.0], [2.0, 0.0, 3.0], [4.0, 0.0, 3.0], [6.0, 2.0, 3.0]])
    vel = np.array([[2.0, 0.0, 0.0]] * 3 + [[0.0, 2.0, 0.0]])
    p, v = sarx.reference_geometry(pos, vel, np.array([0.0, 1.0, 2.0, 4.0]), (2.0, 6.0))       # mean 1.75
    assert np.allclose(p, [3.5 + 2.0, 0.0, 3.0]) and np.allclose(v, [2.0, 0.0, 0.0])
    p, v = sarx.reference_geometry(pos, vel, np.array([0.0, 1.0, 2.0, 3.0]))
    assert np.allclose(p, [3.0, 0.0, 3.0])
    with pytest.raises(ValueError):
        sarx.reference_geometry(pos, vel[:3], np.arange(4.0))
    with pytest.raises(ValueError):
        sarx.reference_geometry(pos, vel * 0, np.arange(4.0))


def test_relocate_entry_points_under_address_and_ub_sanitizer():
    """The stand-alone driver (its own main, against libsarx_asan.so), built and run on the CPU."""
    r = subprocess.run(["make", "-j8", "asan-relocate"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "relocate_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_driver_names_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "relocate_asan_test.cpp")).read()
    code = re.sub(r"//[^\n]*", "", drv)                               # a name in a comment does not count
    missing = [n for n in _symbols() if not re.search(r"\b" + n + r"\b", code)]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------------
# the geometry of the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _at(q, v_los, P, V, out=(-1e6, -1e6, 1.0, 1.0, 2000000, 2000000), **kw):
    """relocate() of the one continuous image position q: a grid whose pixel (0, 0) lies there."""
    rec, aux = ref.relocate([(0, 0)], [v_los], P, V, (q[0], q[1], 1.0, 1.0), out, **kw)
    return rec[0], aux


def test_round_trip_through_the_image_position():
    """1000 seeded (g, v_los, P, V), half from the orbit arc (R about 5e5 m, 7 km/s) and half from a 5 km circle at 3 km height
    (100 m/s): relocate(image_position(g)) = g and the range is kept, both within 1e-6 m.  The bound: fp64 rounding 1.1e-16 x 5e5 m
    x about 1e2 of amplification through the difference rho2 - al^2 is about 1e-8 m; 1e-6 leaves two decades."""
    rng = np.random.default_rng(2024)
    k = tb.scaled_constants()
    worst = [0.0, 0.0]
    done = {"orbit": 0, "circle": 0}
    for n in range(1000):
        if n % 2 == 0:
            pos, vel = tb.orbit_arc(np.array([rng.uniform(-2.0, 2.0)]), k)
            P, V, kind = pos[0], vel[0], "orbit"
        else:
            P, V = ref.circle_geometry(rng.uniform(0, 360), speed=rng.uniform(60, 140))
            kind = "circle"
        g = rng.uniform(-1000, 1000, 2)
        v_los = rng.uniform(-15, 15)
        q = ref.image_position(g, v_los, P, V)
        assert q is not None, (n, kind)
        rec, _ = _at(q, v_los, P, V)
        assert rec["status"] == ref.OK, (n, kind, rec)
        back = float(np.hypot(rec["x"] - g[0], rec["y"] - g[1]))
        r_g = np.linalg.norm([g[0] - P[0], g[1] - P[1], P[2]])
        r_q = np.linalg.norm([q[0] - P[0], q[1] - P[1], P[2]])
        worst = [max(worst[0], back), max(worst[1], abs(r_g - r_q))]
        assert back <= 1e-6 and abs(r_g - r_q) <= 1e-6, (n, kind, back, r_g - r_q)
        assert abs(rec["shift_x"] - (g[0] - q[0])) <= 1e-6 and abs(rec["shift_y"] - (g[1] - q[1])) <= 1e-6
        done[kind] += 1
    print(f"worst position error {worst[0]:.2e} m, worst range difference {worst[1]:.2e} m over {done}")
    assert done == {"orbit": 500, "circle": 500}


def test_each_status_the_side_rule_and_the_velocity_solve():
    P, V = np.array([0.0, -4000.0, 3000.0]), np.array([100.0, 0.0, 0.0])            # flying along +x, the scene to its left (n = +y)
    grid = (-180.0, -180.0, 4.0, 5.0)
    out = (-1000.0, -1000.0, 2.0, 2.0, 1000, 1000)
    ij = [(36, 45)] * 7
    v = [2.0, np.nan, np.inf, 2.0, 200.0, -12.0, 0.0]
    valid = [0, 0, 0, 7, 0, 0, 0]
    rec, aux = ref.relocate(ij, v, P, V, grid, out, valid=valid)
    # R = 5000 m at q = (0, 0): v_los 2 m/s shifts 100 m along track; 200 m/s would need al = 10 km > rho = 4 km; -12 m/s lands at
    # x = -600 - within the output grid - and a zero speed changes nothing
    assert rec["status"].tolist() == [ref.OK, ref.NO_SPEED, ref.NO_SPEED, ref.NO_SPEED, ref.NO_SOLUTION, ref.OK, ref.OK]
    assert abs(rec["x"][0] - 100.0) < 1e-9 and abs(rec["shift_x"][0] - 100.0) < 1e-9 and abs(rec["x"][5] + 600.0) < 1e-9
    assert abs(np.hypot(rec["x"][0], rec["y"][0] + 4000.0) - 4000.0) < 1e-9                     # the ground range is kept
    assert rec["shift_x"][6] == 0.0 and abs(rec["shift_y"][6]) < 1e-9
    for r in (1, 2, 3, 4):
        assert all(rec[f][r] == 0 for f in ("x", "y", "shift_x", "shift_y", "vx", "vy", "flags")) and rec["rank"][r] == -1
    rec, _ = ref.relocate([(36, 45)], [-12.0], P, V, grid, (-500.0, -500.0, 2.0, 2.0, 500, 500))
    assert rec["status"][0] == ref.OFF_GRID and abs(rec["x"][0] + 600.0) < 1e-9 and rec["shift_x"][0] != 0.0
    assert ref.relocate([(36, 45)], [2.0], P, [0.0, 0.0, 5.0], grid, out)[0]["status"][0] == ref.NO_SOLUTION      # s2 == 0
    assert ref.relocate([(0, 0)], [2.0], [-180.0, -180.0, 3000.0], V, grid, out)[0]["status"][0] == ref.NO_SOLUTION  # rho2 == 0
    # the side rule: the same image offsets on either side of the track stay on their side
    for sign in (1.0, -1.0):
        q = (30.0, -4000.0 + sign * 3000.0)
        r1, _ = _at(q, 3.0, P, V)
        assert r1["status"] == ref.OK and np.sign(r1["y"] + 4000.0) == sign and abs(r1["x"] - (30.0 + 3.0 * np.hypot(np.hypot(30.0, 3000.0), 3000.0) / 100.0)) < 1e-9
        back = ref.image_position((r1["x"], r1["y"]), 3.0, P, V)
        assert abs(back[0] - q[0]) < 1e-9 and abs(back[1] - q[1]) < 1e-9
    # the velocity solve: a target with ground velocity u gives v_los = u . los and v_along = u . a; both come back
    for u in ((3.0, 4.0), (-7.0, 1.5), (0.0, -9.0)):
        g = np.array([200.0, -300.0])
        los = np.array([g[0] - P[0], g[1] - P[1], -P[2]])
        los /= np.linalg.norm(los)
        v_los = u[0] * los[0] + u[1] * los[1]
        q = ref.image_position(g, v_los, P, V)
        r1, aux = _at(q, v_los, P, V, v_along=[u[0]])
        assert r1["flags"] == ref.HAS_VELOCITY and abs(r1["vx"] - u[0]) < 1e-9 and abs(r1["vy"] - u[1]) < 1e-9, (u, r1)
        r2, _ = _at(q, v_los, P, V, v_along=[np.nan])
        assert r2["flags"] == 0 and r2["vx"] == 0 and r2["vy"] == 0 and r2["x"] == r1["x"]
    # no determinant: the line of sight's ground projection runs along the track
    r3, aux = _at((500.0, -4000.0), 0.0, P, V, v_along=[5.0])
    assert r3["status"] == ref.OK and r3["flags"] == 0 and r3["vx"] == 0 and r3["vy"] == 0


def test_the_output_slot_is_sorted_by_pixel_then_report_and_copies_the_bytes():
    P, V = np.array([0.0, -4000.0, 3000.0]), np.array([100.0, 0.0, 0.0])
    grid, out = (-180.0, -180.0, 4.0, 5.0), (-400.0, -400.0, 8.0, 8.0, 100, 100)
    rng = np.random.default_rng(1)
    rep = np.zeros(6, ref.REPORT_DTYPE)
    rep["i"], rep["j"] = [40, 36, 36, 10, 36, 36], [45, 45, 45, 80, 46, 45]
    for f in ("power", "mean", "interf_re", "interf_im", "mag1", "mag2"):
        rep[f] = rng.uniform(1, 2, 6)
    v = [1.0, 1.0, 1.0, np.nan, 1.0, 1.0]
    rec, aux = ref.relocate(np.stack([rep["i"], rep["j"]], 1), v, P, V, grid, out)
    raw, rec = ref.out_slot(rep, rec, aux, 8)
    assert raw[:8].view("<u4").tolist() == [5, 0] and rec["rank"].tolist() == [4, 0, 1, -1, 3, 2]      # 1, 2, 5 share a pixel: by r
    got = raw[16:16 + 48 * 5].view(ref.REPORT_DTYPE)
    assert got["i"].tolist() == sorted(got["i"].tolist())
    for r, k in enumerate(rec["rank"]):
        if k >= 0:
            assert got[k]["power"] == rep[r]["power"] and got[k]["mag2"] == rep[r]["mag2"]
    assert not raw[16 + 48 * 5:].any()


# ---------------------------------------------------------------------------------------------------------------------
# the restatement's physics: what the feature is for
# ---------------------------------------------------------------------------------------------------------------------
def physics_case(vy):
    """The mover's peak of |I0 - I1| on the restatement's images, relocated by the restated closed form with the restated
    resolver's speed and with the true one."""
    import sarx
    sc = mref.three_rx_scene(vy)
    img = mref.three_rx_images(vy)
    size, nx, ny = mref.GRID
    x0, y0, dx, dy = ref.tdbp_grid(size, nx, ny)
    i, j = ref.mover_peak(img)
    rec = mref.resolve(img, [(i, j)], sc["lags"], sc["wavelength"], 30.0)[0]
    assert rec["status"] == 0
    P, V = sarx.reference_geometry(sc["pos"], sc["vel"], sc["t_vec"], sc["rx_offsets"][:2])
    v_true = mref.v_los_true(sc, vy)
    wide = (-2000.0, -2000.0, dx, dy, 4000, 4000)
    got, _ = ref.relocate([(i, j)], [rec["v_los"]], P, V, (x0, y0, dx, dy), wide)
    exact, _ = ref.relocate([(i, j)], [v_true], P, V, (x0, y0, dx, dy), wide)
    on_chip, _ = ref.relocate([(i, j)], [rec["v_los"]], P, V, (x0, y0, dx, dy), (x0, y0, dx, dy, nx, ny))
    return dict(peak=(i, j), P=P, V=V, v_rec=float(rec["v_los"]), v_true=v_true, got=got[0], exact=exact[0], on_chip=int(on_chip["status"][0]))


@pytest.fixture(scope="module")
def displacement():
    return ref.scatterer_displacement()


@pytest.mark.parametrize("vy", [16.0, -10.0])
def test_a_mover_is_put_back_where_it_is(vy, displacement):
    """three_rx_scene(vy): the peak of |I0 - I1| with the speed of the restated resolver, relocated by the restated closed form.
    Measured: v_y = 16: 4.97 m against a bound of 7.51 m along track (4.04 m of pixel, 3.47 m of speed error); v_y = -10: 11.09
    against 13.55 m; 0.83 and 0.31 m against a row of 5.22 m across; with the true speed both land within a pixel.  Unrelocated the
    error is 788 m and 495 m."""
    b, at = displacement
    print(f"the stationary scatterer peaks at pixel {at} = ({b[0]:.2f}, {b[1]:.2f}) m")
    c = physics_case(vy)
    assert c["got"]["status"] == ref.OK and c["on_chip"] == ref.OFF_GRID      # the mover is off the chip it was imaged on
    f = ref.physics_figures(vy, c["peak"], (c["got"]["x"], c["got"]["y"]), c["v_rec"], c["v_true"], c["P"], c["V"], b)
    print(ref.physics_line(f))
    assert abs(f["slope"] - 66.1) < 0.5
    assert f["err"][0] <= f["bound"][0] and f["err"][1] <= f["bound"][1]
    assert f["before"][0] > 0.9 * 49.5 * abs(vy) and f["before"][0] > 30 * f["bound"][0]         # what was gained
    e = ref.physics_figures(vy, c["peak"], (c["exact"]["x"], c["exact"]["y"]), c["v_true"], c["v_true"], c["P"], c["V"], b)
    assert np.all(e["err"] <= e["bound"]) and np.all(e["bound"] == e["spacing"]), e
