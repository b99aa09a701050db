"""CPU checks of the Kalman ground tracker (include/sarx_ktrack.h, csrc/ktrack.hip, sarx/ktrack.py): header, binding and exported
symbols, every refusal that needs no device, the sanitizer driver, and the filter's consistency, worth, gate and rules on the NumPy
restatement (tests/_ktrack_numpy.py, which tests/test_gpu_ktrack.py holds the kernels to)."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ktrack_numpy as ref  # noqa: E402
import _track_numpy as tref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_ktrack.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")
NAMES = ("sarx_ktrack_check", "sarx_ktrack_table_bytes", "sarx_ktrack_workspace_bytes", "sarx_ktrack_init_dev", "sarx_ktrack_step_dev",
         "sarx_ktrack_run_dev")
INVALID = -1
PARAM_OFFSETS = [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76]
FRAME_OFFSETS = [0, 8, 32, 56, 60]
HEADER_OFFSETS = [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48]
SLOT_OFFSETS = [0, 8, 16, 24, 32, 112, 120, 128, 136, 144, 152, 160, 164, 168, 172, 176, 180, 184, 188]


def _symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


# ---------------------------------------------------------------------------------------------------------------------
# header and binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    import sarx
    from sarx import _ffi, ktrack
    syms = _symbols()
    assert syms == sorted(_ffi.KTRACK_SIGNATURES) == sorted(NAMES)
    assert not set(syms) & set(_ffi.SIGNATURES)                       # sarx.h got no new function
    assert "ktrack" not in open(os.path.join(ROOT, "include", "sarx.h")).read()
    P, F, H, S = _ffi.KtrackParams, _ffi.KtrackFrame, _ffi.KtrackHeader, _ffi.KtrackSlot
    assert (C.sizeof(P), C.sizeof(F), C.sizeof(H), C.sizeof(S)) == (80, 64, 64, 192)
    for T, want in ((P, PARAM_OFFSETS), (F, FRAME_OFFSETS), (H, HEADER_OFFSETS), (S, SLOT_OFFSETS)):
        assert [getattr(T, n).offset for n, _ in T._fields_] == want, T
    for dt, T, other in ((ktrack.HEADER_DTYPE, H, ref.HEADER_DTYPE), (ktrack.SLOT_DTYPE, S, ref.SLOT_DTYPE)):
        assert [n for n, _ in T._fields_] == list(dt.names) and dt == other
        assert [dt.fields[n][1] for n in dt.names] == [getattr(T, n).offset for n, _ in T._fields_]
    assert (_ffi.KTRACK_OK, _ffi.KTRACK_ERR_SLOT_OVERFLOW, _ffi.KTRACK_ERR_TABLE_OVERFLOW, _ffi.KTRACK_ERR_TIME) == \
        (ref.OK, ref.SLOT_OVERFLOW, ref.TABLE_OVERFLOW, ref.TIME) == (0, 1, 2, 3)
    assert (_ffi.KTRACK_FREE, _ffi.KTRACK_TENTATIVE, _ffi.KTRACK_CONFIRMED) == (ref.FREE, ref.TENTATIVE, ref.CONFIRMED) == (0, 1, 2)
    assert (_ffi.KTRACK_MAX_TRACKS, _ffi.KTRACK_MAX_DETECTIONS) == (_ffi.TRACK_MAX_TRACKS, _ffi.TDBP_MULTI_MAX_DETECTIONS)
    lib = _ffi.load()
    assert lib.sarx_version() == 206
    for s in NAMES:
        assert hasattr(lib, s), s
    for name in ("ground_track", "GroundTracker", "KalmanTrackParams", "KalmanTrackResult", "TrackTimeError"):
        assert name in sarx.__all__ and hasattr(sarx, name)
    assert issubclass(sarx.TrackTimeError, sarx.SarxError) and not issubclass(sarx.TrackTimeError, sarx.TrackOverflowError)
    cp = sarx.KalmanTrackParams(max_tracks=5, max_detections=7).c_params()
    assert ktrack.table_bytes(cp) == 64 + 192 * 5
    assert ktrack.workspace_bytes(cp) == 8 * (15 * 256 + 11 * 256) + 4 * (2 * 256 + 256)
    assert "sarx_ktrack.h" in open(os.path.join(ROOT, "include", "sarx_track.h")).read()      # its "Left out" points here


def test_header_is_c99(tmp_path):
    checks = ["sizeof(sarx_ktrack_params) == 80", "sizeof(sarx_ktrack_frame) == 64", "sizeof(sarx_ktrack_header) == 64",
              "sizeof(sarx_ktrack_slot) == 192"]
    for T, names, offs in (("params", ("sigma_pos", "sigma_v", "sigma_v_tan", "q", "gate_d2", "gate_m", "birth_ratio", "confirm_hits",
                                       "confirm_window", "max_misses", "max_tracks", "max_detections", "reserved"), PARAM_OFFSETS),
                           ("frame", ("t", "pos_ref", "vel_ref", "frame_index", "reserved"), FRAME_OFFSETS),
                           ("header", ("n_live", "n_confirmed", "next_id", "frames_done", "births_total", "drops_total", "error", "error_frame",
                                       "max_tracks", "reserved0", "t_last", "reserved"), HEADER_OFFSETS),
                           ("slot", ("x", "y", "vx", "vy", "p", "sum_re", "sum_im", "sum_power", "max_ratio", "nis_last", "nis_sum", "id", "status",
                                     "hits", "misses", "age", "hist", "last_frame", "last_report"), SLOT_OFFSETS)):
        checks += [f"offsetof(sarx_ktrack_{T}, {n}) == {o}" for n, o in zip(names, offs)]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "sarx_ktrack.h"\nint main(void) { return ' + " && ".join(checks) + " ? 0 : 1; }\n")
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
GOOD = dict(sigma_pos=1.0, sigma_v=0.3, sigma_v_tan=10.0, q=0.01, gate_d2=16.27, gate_m=100.0, birth_ratio=0.0, confirm_hits=3,
            confirm_window=5, max_misses=3, max_tracks=1024, max_detections=4096, reserved=0)


def _params(**kw):
    from sarx import _ffi
    return _ffi.KtrackParams(*dict(GOOD, **kw).values())


def _refused(rc, word):
    from sarx import _ffi
    msg = _ffi.load().sarx_last_error(None).decode()
    assert rc == INVALID and word in msg, (rc, msg, word)


def test_every_refusal_of_the_parameter_check():
    from sarx import _ffi
    lib = _ffi.load()
    chk = lib.sarx_ktrack_check
    assert chk(C.byref(_params())) == 0
    assert chk(C.byref(_params(q=0.0, birth_ratio=1e300, sigma_pos=1e-300, confirm_hits=32, confirm_window=32, max_misses=0,
                               max_tracks=_ffi.KTRACK_MAX_TRACKS, max_detections=_ffi.KTRACK_MAX_DETECTIONS))) == 0
    assert chk(C.byref(_params(confirm_hits=1, confirm_window=1, max_tracks=1, max_detections=1))) == 0
    _refused(chk(None), "NULL")
    for name in ("sigma_pos", "sigma_v", "sigma_v_tan", "gate_d2", "gate_m"):
        for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            _refused(chk(C.byref(_params(**{name: bad}))), name + " ")
    for name in ("q", "birth_ratio"):
        for bad in (-1e-300, -1.0, float("nan"), float("inf"), -float("inf")):
            _refused(chk(C.byref(_params(**{name: bad}))), name + " ")
    for n in (0, -1, 33):
        _refused(chk(C.byref(_params(confirm_window=n, confirm_hits=1))), "confirm_window")
    for m in (0, -1, 6):
        _refused(chk(C.byref(_params(confirm_hits=m))), "confirm_hits")
    _refused(chk(C.byref(_params(max_misses=-1))), "max_misses")
    for n in (0, -1, _ffi.KTRACK_MAX_TRACKS + 1, 2 ** 31 - 1):
        _refused(chk(C.byref(_params(max_tracks=n))), "max_tracks")
    for n in (0, -1, _ffi.KTRACK_MAX_DETECTIONS + 1, 2 ** 31 - 1):
        _refused(chk(C.byref(_params(max_detections=n))), "max_detections")
    for r in (1, -1):
        _refused(chk(C.byref(_params(reserved=r))), "reserved")
    n = C.c_size_t(12345)
    for fn in (lib.sarx_ktrack_table_bytes, lib.sarx_ktrack_workspace_bytes):
        _refused(fn(C.byref(_params(gate_m=0.0)), C.byref(n)), "gate_m")
        assert n.value == 12345
        _refused(fn(C.byref(_params()), None), "NULL")
    # without a context the device entry points refuse before they read anything
    fr = _ffi.KtrackFrame()
    _refused(lib.sarx_ktrack_init_dev(None, C.byref(_params()), None), "ctx")
    _refused(lib.sarx_ktrack_step_dev(None, C.byref(_params()), C.byref(fr), None, None, None, 8, None, None, None), "ctx")
    _refused(lib.sarx_ktrack_run_dev(None, C.byref(_params()), C.byref(fr), 1, None, 0, None, 0, None, 8, 0, None, None, None), "ctx")


def test_python_parameters_check_before_any_device_work():
    import sarx
    p = sarx.KalmanTrackParams()
    cp = p.c_params()
    assert (cp.sigma_pos, cp.sigma_v, cp.sigma_v_tan, cp.gate_d2, cp.confirm_hits, cp.confirm_window, cp.reserved) == (1.0, 0.3, 10.0, 16.27, 3, 5, 0)
    assert p.slot_bytes() == 16 + 48 * 4096
    for bad in (dict(sigma_pos=0.0), dict(sigma_v=-1.0), dict(sigma_v_tan=float("nan")), dict(q=-1.0), dict(gate_d2=0.0), dict(gate_m=float("inf")),
                dict(birth_ratio=-1.0), dict(confirm=(4, 3)), dict(confirm=(1, 33)), dict(confirm=3), dict(max_misses=-1), dict(max_tracks=0),
                dict(max_detections=16385)):
        with pytest.raises(ValueError):
            sarx.KalmanTrackParams(**bad).check()
    from sarx.ktrack import c_frame
    f = c_frame(2.5, (1, 2, 3), (4, 5, 6), 7)
    assert (f.t, list(f.pos_ref), list(f.vel_ref), f.frame_index, f.reserved) == (2.5, [1, 2, 3], [4, 5, 6], 7, 0)
    with pytest.raises(ValueError):
        c_frame(0.0, (1, 2), (4, 5, 6), 0)


def test_ktrack_entry_points_under_address_and_ub_sanitizer():
    """The stand-alone driver (its own main, against libsarx_asan.so), built and run on the CPU."""
    r = subprocess.run(["make", "-j8", "asan-ktrack"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "ktrack_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_driver_names_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "ktrack_asan_test.cpp")).read()
    code = re.sub(r"//[^\n]*", "", drv)                               # a name in a comment does not count
    missing = [n for n in _symbols() if not re.search(r"\b" + n + r"\b", code)]
    assert not missing, missing


# ---------------------------------------------------------------------------------------------------------------------
# what the filter is for: consistency, and worth over the existing tracker
# ---------------------------------------------------------------------------------------------------------------------
SCENE = dict(q=1e-9, sigma_pos=1.0, sigma_v=0.3, sigma_v_tan=10.0, gate_d2=50.0, gate_m=150.0, max_tracks=512, max_detections=512)
N_MOVERS, N_FRAMES = 400, 16


def _own_ids(tr):
    """Every mover is born in frame 0 under its own index and keeps it: no innovation in the statistics is a wrong pairing."""
    return all(np.array_equal(row[:N_MOVERS], np.arange(N_MOVERS)) for row in tr.assoc)


def test_the_innovations_are_consistent():
    """400 movers x 16 frames on the 5 km circle (3 km height, 5 degrees and 2 s per frame), sigma_pos = 1 m, sigma_v = 0.3 m/s, q =
    1e-9, true velocities N(0, 10^2 I) = the birth prior, measurements drawn through J at the true position.  The mean of the M = 6000
    innovations' d2 must lie within five standard deviations of a chi-square-3 mean: 3 +- 5 sqrt(6 / M) = [2.84, 3.16].  Measured:
    3.11 (the gate of 50 cuts 1e-10 of a chi-square-3; the filter linearises u and k at the measured position, the draws use the true
    one)."""
    frames, _ = ref.mover_scene(N_MOVERS, N_FRAMES, seed=3)
    tr = ref.run(frames, ref.params(**SCENE))
    assert _own_ids(tr) and int(tr.hdr["n_live"]) == N_MOVERS
    m = len(tr.nis)
    assert m == 6000
    mean = float(np.mean(tr.nis))
    half = 5.0 * np.sqrt(6.0 / m)
    print(f"mean NIS {mean:.3f} over {m} innovations, allowed 3 +- {half:.3f}")
    assert abs(mean - 3.0) <= half


@pytest.fixture(scope="module")
def worth():
    """The same scene with speeds of 3 - 15 m/s at uniform headings: the Kalman restatement, and the existing tracker's restatement
    (tests/_track_numpy.py) on the same reports rounded to a ground grid of 8 m pixels with a gate of 8 pixels (the largest step, 30
    m, plus the 2.5 pixels of along-track noise and quantisation), its pixel-per-frame velocity converted by out_dx / dt, for each
    (alpha, beta) of {0.3, 0.5, 0.8} x {0.1, 0.2, 0.4}."""
    frames, truth = ref.mover_scene(N_MOVERS, N_FRAMES, seed=4, speeds=(3.0, 15.0))
    tr = ref.run(frames, ref.params(**SCENE))
    assert _own_ids(tr)
    v = np.stack([tr.slots["vx"][:N_MOVERS], tr.slots["vy"][:N_MOVERS]], axis=1)
    kalman = float(np.sqrt(np.mean(np.sum((v - truth["vel"]) ** 2, axis=1))))
    dx, dt, x0 = 8.0, ref.CIRCLE["dt"], -8192.0
    old_frames, where = [], None
    for fr in frames:
        ij = np.stack([np.rint((fr["rec"]["y"] - x0) / dx), np.rint((fr["rec"]["x"] - x0) / dx)], axis=1).astype(np.int64)
        rep = tref.make_reports(ij)
        key = {(int(a), int(b)): r for r, (a, b) in enumerate(zip(rep["i"], rep["j"]))}
        where = np.array([key[(int(a), int(b))] for a, b in ij])      # the mover's report in this frame's sorted list
        old_frames.append(rep)
    old = {}
    for alpha in (0.3, 0.5, 0.8):
        for beta in (0.1, 0.2, 0.4):
            t = tref.run(old_frames, tref.params(gate_az=8.0, gate_rg=8.0, alpha=alpha, beta=beta, max_tracks=1024, max_detections=512))
            s = t.slots
            by_report = {int(s["last_report"][k]): k for k in np.flatnonzero((s["status"] != tref.FREE) & (s["last_frame"] == N_FRAMES - 1))}
            held = np.array([m for m in range(N_MOVERS) if int(where[m]) in by_report])
            k = np.array([by_report[int(where[m])] for m in held])
            vo = np.stack([s["v_j"][k], s["v_i"][k]], axis=1) * dx / dt
            old[(alpha, beta)] = (float(np.sqrt(np.mean(np.sum((vo - truth["vel"][held]) ** 2, axis=1)))), len(held))
    return kalman, old


def test_worth_over_the_existing_tracker(worth):
    """Velocity RMS error (both components, m/s) at the last frame.  Measured: Kalman 0.057; the existing tracker's best of the nine
    (alpha, beta) 0.567 at (0.5, 0.1), the others 1.09 - 3.07, each holding 395 - 398 of the 400 movers to the end."""
    kalman, old = worth
    for k, (rms, held) in sorted(old.items()):
        print(f"alpha-beta {k}: {rms:.3f} m/s over {held} movers")
        assert held >= 0.9 * N_MOVERS
    best = min(rms for rms, _ in old.values())
    print(f"Kalman {kalman:.3f} m/s against the existing tracker's best {best:.3f} m/s")
    assert kalman < best


# ---------------------------------------------------------------------------------------------------------------------
# the gate is the ellipse
# ---------------------------------------------------------------------------------------------------------------------
def _one_report(z, v, P, V, t, **kw):
    return dict(reports=ref.make_reports(1), rec=ref.make_records([z], **kw), v_los=np.array([v]), t=t, P=P, V=V)


def _decision(tr, p, z, v, f):
    """(what the restatement's step decides, what S says) for one report at z with speed v in frame f against the one live track."""
    P, V = ref.frame_geometry(f)
    t = ref.CIRCLE["dt"] * f
    s = tr.slots[0]
    xm, Pm = ref.predict(np.array([[s["x"], s["y"], s["vx"], s["vy"]]]), s["p"][None, :], t - float(tr.hdr["t_last"]), p["q"])
    rec = ref.make_records([z])
    ok, meas = ref.measurements(rec, [v], P, V, p)
    assert ok[0]
    inn = ref.innovation(xm[0], Pm[0], meas[0])
    S = ref.s_matrix(inn)
    nu = np.array([float(x) for x in inn["nu"]])
    d2 = float(nu @ np.linalg.solve(S, nu))
    assert abs(d2 - p["gate_d2"]) > 1e-3 * p["gate_d2"] and abs(abs(nu[0]) - p["gate_m"]) > 1e-3 and abs(abs(nu[1]) - p["gate_m"]) > 1e-3
    expect = bool(d2 <= p["gate_d2"] and abs(nu[0]) <= p["gate_m"] and abs(nu[1]) <= p["gate_m"])
    trial = copy.deepcopy(tr)
    row = trial.step(ref.make_reports(1), rec, [v], dict(t=t, P=P, V=V, index=f))
    return bool(row[0] == s["id"]), expect, d2, S, (xm[0], meas[0])


def test_the_gate_is_the_ellipse_and_turns_with_the_aspect():
    """One track, born in frame 0.  In frame 1 a report displaced D = 2 sqrt(S_along) along the track direction a is taken; one
    displaced the same D along the normal n is refused: a box in grid axes that takes the first takes the second.  Each displaced
    report carries the speed innovation S expects with its displacement (S_vp S_pp^-1 dz, the conditional mean: position and speed
    errors are correlated), so that d2 is that of the position ellipse.  The same two displacements, kept in grid axes with their
    speeds, one frame (5 degrees) later are decided by that frame's S.  Every expected decision is nu' S^-1 nu against gate_d2 (and
    |nu| against gate_m), formed here from the restatement's S with a general solver."""
    p = ref.params(q=1e-9, gate_d2=16.27, gate_m=100.0, max_tracks=4, max_detections=4)
    P0, V0 = ref.frame_geometry(0)
    g, vel = np.array([120.0, -60.0]), np.array([6.0, 3.0])
    los = lambda gg, PP: (gg - PP[:2]) / np.sqrt(np.sum((gg - PP[:2]) ** 2) + PP[2] ** 2)      # noqa: E731
    tr = ref.run([_one_report(g, float(vel @ los(g, P0)), P0, V0, 0.0)], p)
    assert int(tr.hdr["n_live"]) == 1
    shifts = {}
    for f in (1, 2):
        P, V = ref.frame_geometry(f)
        s = float(np.hypot(V[0], V[1]))
        a = V[:2] / s
        nrm = np.array([-a[1], a[0]])
        gf = g + vel * ref.CIRCLE["dt"] * f
        # the prediction's own measurement: nu = 0
        st = tr.slots[0]
        dtf = ref.CIRCLE["dt"] * f - float(tr.hdr["t_last"])
        centre = np.array([st["x"] + dtf * st["vx"], st["y"] + dtf * st["vy"]])
        v_centre = float(np.array([st["vx"], st["vy"]]) @ los(centre, P))
        took, expect, d2, S, _ = _decision(tr, p, centre, v_centre, f)
        assert took and expect and d2 < 1e-12
        if f == 1:
            k = float(np.sqrt(np.sum((centre - P[:2]) ** 2) + P[2] ** 2)) / s
            D = 2.0 * float(np.sqrt(a @ S[:2, :2] @ a))
            cond = lambda dz: float(S[2, :2] @ np.linalg.solve(S[:2, :2], dz))      # noqa: E731
            shifts = dict(along=(D * a, cond(D * a)), across=(D * nrm, cond(D * nrm)))
            print(f"frame 1: sqrt(S_along) {D / 2:.2f} m, sqrt(S_across) {float(np.sqrt(nrm @ S[:2, :2] @ nrm)):.2f} m, k {k:.1f} s")
        got = {}
        for name, (dz, dv) in shifts.items():
            took, expect, d2, _, _ = _decision(tr, p, centre + dz, v_centre + dv, f)
            print(f"frame {f}: displaced {name} by ({dz[0]:.1f}, {dz[1]:.1f}) m, {dv:+.2f} m/s: d2 {d2:.2f} -> {'taken' if took else 'refused'}")
            assert took == expect, (f, name, d2)
            got[name] = took
        if f == 1:
            assert got == dict(along=True, across=False)
            assert np.all(np.abs(shifts["across"][0]) < p["gate_m"])      # the coarse box holds both: the ellipse decides
        # the track goes on to the next frame with its own measurement
        tr.step(ref.make_reports(1), ref.make_records([gf]), [float(vel @ los(gf, P))], dict(t=ref.CIRCLE["dt"] * f, P=P, V=V, index=f))
        assert int(tr.hdr["n_live"]) == 1 and tr.assoc[-1][0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# rules and errors
# ---------------------------------------------------------------------------------------------------------------------
def _frame(g, v_true, f, t=None, **kw):
    """Exact measurements of movers at g with velocities v_true in frame f's geometry; kw (status, vel) go to the records."""
    P, V = ref.frame_geometry(f)
    g = np.asarray(g, np.float64).reshape(-1, 2)
    vel = np.asarray(v_true, np.float64).reshape(-1, 2)
    d = g - P[:2]
    u = d / np.sqrt(np.sum(d * d, axis=1) + P[2] ** 2)[:, None]
    out = dict(reports=ref.make_reports(len(g)), rec=ref.make_records(g, **kw), v_los=np.sum(vel * u, axis=1), t=ref.CIRCLE["dt"] * f if t is None else t,
               P=P, V=V)
    return out, u


def test_a_birth_takes_the_measured_component_and_the_given_velocity():
    p = ref.params(max_tracks=8, max_detections=8)
    g = np.array([[100.0, 50.0], [-300.0, 200.0], [40.0, -700.0]])
    vel = np.array([[5.0, -2.0], [-8.0, 1.0], [0.5, 12.0]])
    given = np.array([[np.nan, np.nan], [-8.0, 1.0], [np.nan, np.nan]])
    fr, u = _frame(g, vel, 3, vel=given)
    tr = ref.run([fr], p)
    s = tr.slots[:3]
    assert s["id"].tolist() == [0, 1, 2] and np.all(s["status"] == ref.TENTATIVE) and np.all(s["hits"] == 1) and np.all(s["nis_sum"] == 0)
    assert np.array_equal(s["x"], g[:, 0]) and np.array_equal(s["y"], g[:, 1])
    hx = u[:, 0] * s["vx"] + u[:, 1] * s["vy"]
    assert np.all(np.abs(hx - fr["v_los"]) <= 4 * np.finfo(float).eps * np.abs(fr["v_los"]))       # H x = z at birth
    m = np.hypot(u[:, 0], u[:, 1])
    for k in (0, 2):                                                   # the velocity lies along e and is v / m long, not v m
        assert abs(np.hypot(s["vx"][k], s["vy"][k]) - abs(fr["v_los"][k]) / m[k]) < 1e-12
        assert abs(s["vx"][k] * u[k, 1] - s["vy"][k] * u[k, 0]) < 1e-12
        Pv = np.array([[s["p"][k][7], s["p"][k][8]], [s["p"][k][8], s["p"][k][9]]])
        e = u[k] / m[k]
        assert abs(e @ Pv @ e - (p["sigma_v"] / m[k]) ** 2) < 1e-12 and abs(np.array([-e[1], e[0]]) @ Pv @ np.array([-e[1], e[0]]) - 100.0) < 1e-9
    assert (s["vx"][1], s["vy"][1]) == (-8.0, 1.0) and s["p"][1][7] == s["p"][1][9] == p["sigma_v"] ** 2 and s["p"][1][8] == 0.0
    # P_pos is Rm's position block: sigma_pos across, sqrt(sigma_pos^2 + (k sigma_v)^2) along track
    P, V = fr["P"], fr["V"]
    a = V[:2] / np.hypot(V[0], V[1])
    k0 = np.sqrt(np.sum((g[0] - P[:2]) ** 2) + P[2] ** 2) / np.hypot(V[0], V[1])
    Pp = np.array([[s["p"][0][0], s["p"][0][1]], [s["p"][0][1], s["p"][0][4]]])
    assert abs(a @ Pp @ a - (1.0 + (k0 * 0.3) ** 2)) < 1e-9 and abs(np.array([-a[1], a[0]]) @ Pp @ np.array([-a[1], a[0]]) - 1.0) < 1e-9
    # reports that are no measurement start nothing
    bad, _ = _frame(g, vel, 3, status=[ref.REC_NO_SPEED, ref.REC_NO_SOLUTION, ref.REC_OFF_GRID])
    bad["v_los"][2] = np.nan
    tr = ref.run([bad], p)
    assert int(tr.hdr["n_live"]) == 0 and (tr.assoc[0] == -1).all()
    off, _ = _frame(g, vel, 3, status=[ref.REC_OK, ref.REC_OFF_GRID, ref.REC_NO_SPEED])
    tr = ref.run([off], p)
    assert tr.assoc[0][:3].tolist() == [0, 1, -1]                      # OFF_GRID is solved: this tracker has no grid


def test_ties_go_to_the_smaller_index():
    p = ref.params(max_tracks=8, max_detections=8)
    g, vel = np.array([[100.0, 50.0]]), np.array([[5.0, -2.0]])
    one, _ = _frame(g, vel, 0)
    two, _ = _frame(np.repeat(g + vel * 2.0, 2, axis=0), np.repeat(vel, 2, axis=0), 1)
    tr = ref.run([one, two], p)                                        # two identical reports for one track: the smaller r
    assert tr.assoc[1][:2].tolist() == [0, -1] and int(tr.hdr["n_live"]) == 1
    twins, _ = _frame(np.repeat(g, 2, axis=0), np.repeat(vel, 2, axis=0), 0)
    single, _ = _frame(g + vel * 2.0, vel, 1)
    tr = ref.run([twins, single], p)                                   # two identical tracks for one report: the smaller slot
    assert tr.assoc[0][:2].tolist() == [0, 1] and tr.assoc[1][0] == 0
    assert tr.slots["hits"][:2].tolist() == [2, 1] and tr.slots["misses"][:2].tolist() == [0, 1]


def test_confirmation_drops_and_the_table_overflow():
    p = ref.params(max_tracks=3, max_detections=8, confirm_hits=3, confirm_window=5, max_misses=2)
    g, vel = np.array([[100.0, 50.0]]), np.array([[5.0, -2.0]])
    seen = [1, 1, 0, 1, 0, 0, 0]
    frames = []
    for f, hit in enumerate(seen):
        fr, _ = _frame(g + vel * 2.0 * f, vel, f)
        if not hit:
            fr = dict(fr, reports=ref.make_reports(0), rec=ref.make_records(np.zeros((0, 2))), v_los=np.zeros(0))
        frames.append(fr)
    tr = ref.Tracker(p)
    status = []
    for f, fr in enumerate(frames):
        tr.step(fr["reports"], fr["rec"], fr["v_los"], dict(t=fr["t"], P=fr["P"], V=fr["V"], index=f))
        status.append((int(tr.slots["status"][0]), int(tr.slots["hits"][0]), int(tr.slots["misses"][0])))
    assert status == [(1, 1, 0), (1, 2, 0), (1, 2, 1), (2, 3, 0), (2, 3, 1), (2, 3, 2), (0, 0, 0)]      # confirmed at the third hit, dropped at the third miss
    assert int(tr.hdr["drops_total"]) == 1 and int(tr.hdr["frames_done"]) == 7 and not tr.slots.view(np.uint8).any()
    # a coasting track keeps its velocity and grows its covariance
    tr = ref.run(frames[:3], p)
    assert tr.slots["p"][0][0] > ref.run(frames[:2], p).slots["p"][0][0]
    # three live tracks and a fourth report far away: the table is full, NO birth is made, the matched keep their ids, sticky
    g3 = np.array([[100.0, 50.0], [900.0, 50.0], [100.0, 900.0]])
    v3 = np.zeros((3, 2))
    a, _ = _frame(g3, v3, 0)
    b, _ = _frame(np.concatenate([g3, [[-900.0, -900.0], [-1500.0, 300.0]]]), np.zeros((5, 2)), 1)
    c, _ = _frame(g3, v3, 2)
    tr = ref.run([a, b, c], p)
    assert (int(tr.hdr["error"]), int(tr.hdr["error_frame"]), int(tr.hdr["frames_done"])) == (ref.TABLE_OVERFLOW, 1, 1)
    assert tr.assoc[1][:5].tolist() == [0, 1, 2, -1, -1] and (tr.assoc[2] == -1).all() and tr.slots["hits"].tolist() == [2, 2, 2]
    assert int(tr.hdr["next_id"]) == 3 and int(tr.hdr["births_total"]) == 3


def test_slot_overflow_and_time_errors_are_sticky():
    p = ref.params(max_tracks=4, max_detections=4)
    g, vel = np.array([[100.0, 50.0]]), np.array([[5.0, -2.0]])
    f0, _ = _frame(g, vel, 0)
    f1, _ = _frame(g + vel * 2.0, vel, 1)
    for bad in (dict(f1, overflow=1), dict(f1, count=5), dict(f1, rec=ref.make_records(g, status=[ref.REC_OVERFLOW]))):
        tr = ref.run([f0, bad, f1], p)
        assert (int(tr.hdr["error"]), int(tr.hdr["error_frame"]), int(tr.hdr["frames_done"])) == (ref.SLOT_OVERFLOW, 1, 1)
        assert np.array_equal(tr.slots, ref.run([f0], p).slots) and (tr.assoc[1] == -1).all() and (tr.assoc[2] == -1).all()
    # dt = 0: the prediction is the state, the covariance unchanged, the report taken
    same, _ = _frame(g, vel, 0, t=0.0)
    tr = ref.run([f0, same], p)
    assert int(tr.hdr["error"]) == ref.OK and tr.assoc[1][0] == 0 and tr.slots["hits"][0] == 2 and tr.slots["nis_last"][0] < 1e-20
    # dt < 0 and a dt that is not finite
    for t_bad in (-1e-9, -2.0):
        back, _ = _frame(g, vel, 1, t=t_bad)
        tr = ref.run([f0, back, f1], p)
        assert (int(tr.hdr["error"]), int(tr.hdr["error_frame"]), int(tr.hdr["frames_done"])) == (ref.TIME, 1, 1)
        assert np.array_equal(tr.slots, ref.run([f0], p).slots) and float(tr.hdr["t_last"]) == 0.0 and (tr.assoc[2] == -1).all()
    first, _ = _frame(g, vel, 0, t=-1e308)
    far, _ = _frame(g, vel, 1, t=1e308)
    tr = ref.run([first, far], p)
    assert int(tr.hdr["error"]) == ref.TIME
    # the first step of a table takes any time
    neg, _ = _frame(g, vel, 0, t=-5.0)
    assert int(ref.run([neg], p).hdr["error"]) == ref.OK
