"""CPU checks of the GMTI tracker (include/sarx_track.h, csrc/track.hip, sarx/track.py): the C ABI and its binding, the header as
C99, the sanitizer driver of the new entry points, parameter validation, the NumPy restatement on a seeded scenario, the speed
unwrapping, and that no kernel of track.hip uses scratch."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _track_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_track.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")


def _track_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from sarx import _ffi
    syms = _track_symbols()
    assert syms == sorted(_ffi.TRACK_SIGNATURES), set(syms) ^ set(_ffi.TRACK_SIGNATURES)
    for other in (_ffi.SIGNATURES, _ffi.GMTI_SIGNATURES, _ffi.REFOCUS_SIGNATURES, _ffi.BALANCE_SIGNATURES):
        assert not set(syms) & set(other)
    for name in ("sarx_track_check", "sarx_track_table_bytes", "sarx_track_workspace_bytes", "sarx_track_init_dev", "sarx_track_step_dev",
                 "sarx_track_run_dev"):
        assert name in syms


def test_library_exports_the_track_symbols():
    from sarx import _ffi
    lib = _ffi.load()
    for s in _track_symbols():
        assert hasattr(lib, s), s
    assert lib.sarx_version() == 206                                   # sarx.h and its version stay what they were


def test_struct_layouts():
    from sarx import _ffi, track
    assert C.sizeof(_ffi.TrackParams) == 64 and C.sizeof(_ffi.TrackHeader) == 64 and C.sizeof(_ffi.TrackSlot) == 96
    for struct, dtype in ((_ffi.TrackHeader, track.HEADER_DTYPE), (_ffi.TrackSlot, track.SLOT_DTYPE),
                          (_ffi.TrackHeader, ref.HEADER_DTYPE), (_ffi.TrackSlot, ref.SLOT_DTYPE)):
        assert dtype.itemsize == C.sizeof(struct) and dtype.itemsize % 16 == 0
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name
    assert _ffi.TrackHeader.error.offset == 24 and _ffi.TrackSlot.id.offset == 64 and _ffi.TrackParams.confirm_hits.offset == 40


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sarx_track.h"\nint main(void) { sarx_track_slot s; sarx_track_header h; sarx_track_params p; '
                   '(void)s; (void)h; (void)p; return (int)sizeof(sarx_track_slot) - 96 + (int)sizeof(sarx_track_header) - 64 + '
                   '(int)sizeof(sarx_track_params) - 64; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HDR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_track_entry_points_under_address_and_ub_sanitizer():
    r = subprocess.run(["make", "-j8", "asan-track"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "track_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_track_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "track_asan_test.cpp")).read()
    missing = [n for n in _track_symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing


def test_parameter_validation():
    import sarx
    from sarx import _ffi, track
    for bad in (dict(gate=(0.0, 4.0)), dict(gate=(4.0, -1.0)), dict(gate=4.0), dict(gate=(float("inf"), 1.0)), dict(alpha=0.0),
                dict(alpha=1.5), dict(beta=-0.1), dict(beta=2.5), dict(confirm=(0, 5)), dict(confirm=(6, 5)), dict(confirm=(3, 33)),
                dict(max_misses=-1), dict(birth_ratio=-1.0), dict(birth_ratio=float("nan")), dict(max_tracks=0),
                dict(max_tracks=16385), dict(max_detections=0)):
        with pytest.raises(ValueError):
            sarx.TrackParams(**bad).c_params()
        with pytest.raises(ValueError):
            sarx.gmti_track([], sarx.TrackParams(**bad), frame_dt_s=0.1)
    with pytest.raises(ValueError):
        sarx.gmti_track([], sarx.TrackParams(), frame_dt_s=0.0)
    from sarx.batch import TwoChannelBatch
    with pytest.raises(ValueError, match="track"):
        TwoChannelBatch(None, 64, 2, stack="multilook", track=sarx.TrackParams())
    # the library's own check, past the host's
    lib = _ffi.load()
    cp = sarx.TrackParams(confirm=(1, 32), alpha=1.0, beta=2.0, max_tracks=16384, max_detections=1000).c_params()
    assert lib.sarx_track_check(C.byref(cp)) == 0
    assert track.table_bytes(cp) == 64 + 96 * 16384
    assert track.workspace_bytes(cp) == 4 * (2 * 16384 + 1000)
    cp.max_detections = 1001                                           # every array of the workspace a multiple of 16 bytes
    assert track.workspace_bytes(cp) == 4 * (2 * 16384 + 1004)
    for field, value in (("gate_az", 0.0), ("alpha", 1.5), ("beta", -1.0), ("confirm_hits", 33), ("confirm_window", 0), ("max_misses", -1),
                         ("max_tracks", 16385), ("max_detections", 0), ("reserved", 1), ("birth_ratio", float("nan"))):
        cp = sarx.TrackParams().c_params()
        setattr(cp, field, value)
        assert lib.sarx_track_check(C.byref(cp)) != 0, field
        assert len(lib.sarx_last_error(None)) > 10
    assert lib.sarx_track_check(None) != 0


def test_encode_and_decode():
    from sarx import gmti, track
    rep = ref.make_reports([[5, 7], [2, 9], [5, 3]])
    raw = track.encode_slot(rep.astype(gmti.REPORT_DTYPE), 8)
    assert raw.size == 16 + 48 * 8 and np.array_equal(raw, ref.slot_bytes(rep, 8))
    assert np.array_equal(track.encode_slot(raw[:16 + 48 * 3], 8), raw)           # a trimmed slot is padded
    with pytest.raises(gmti.GmtiOverflowError):
        track.encode_slot(rep.astype(gmti.REPORT_DTYPE), 2)
    tr = ref.run([rep, rep], ref.params(max_tracks=4, max_detections=8, confirm_hits=2, confirm_window=3))
    res = track.TrackResult(tr.table_bytes(), np.stack(tr.assoc), [np.stack([rep["i"], rep["j"]], 1)] * 2, 0.1, 2.0, 50.0)
    assert res.n_live == 3 and res.n_confirmed == 3 and res.tracks["id"].tolist() == [0, 1, 2] and sorted(res.paths) == [0, 1, 2]
    assert res.paths[1] == dict(frames=[0, 1], reports=[1, 1], i=[5, 5], j=[3, 3])
    assert np.all(res.tracks["range_rate_mps"] == 0.0)
    tr.hdr["error"], tr.hdr["error_frame"] = ref.TABLE_OVERFLOW, 1
    with pytest.raises(track.TrackOverflowError) as e:
        track.TrackResult(tr.table_bytes(), np.stack(tr.assoc), [np.zeros((0, 2))] * 2)
    assert e.value.kind == "table" and e.value.frame == 1


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------
def test_restatement_rules_by_hand():
    """A tentative track confirms at M of N, coasts on p + v, drops after max_misses + 1 misses, frees its slot for a birth in the
    same step, and a report in the gate of a track that did not take it starts nothing."""
    p = ref.params(max_tracks=2, max_detections=8, gate_az=4.0, gate_rg=4.0, alpha=0.5, beta=0.5, confirm_hits=2, confirm_window=3,
                   max_misses=1)
    t = ref.Tracker(p)
    assert t.step(ref.make_reports([[10, 10]]), 0).tolist()[:2] == [0, -1]
    t.step(ref.make_reports([[12, 10], [13, 12]]), 1)                 # both in the gate: the nearer is taken, the other starts nothing
    assert t.assoc[1][:2].tolist() == [0, -1] and t.hdr["n_live"] == 1 and t.hdr["n_confirmed"] == 1
    s = t.slots[0]
    assert (s["p_i"], s["v_i"], s["hits"], s["hist"], s["age"]) == (11.0, 1.0, 2, 3, 2)
    t.step(ref.make_reports([]), 2)
    assert t.slots[0]["p_i"] == 12.0 and t.slots[0]["misses"] == 1
    t.step(ref.make_reports([[100, 100], [200, 200]]), 3)              # second miss: dropped, and its slot taken in the same step
    assert t.hdr["drops_total"] == 1 and t.hdr["n_live"] == 2 and t.slots["id"].tolist() == [1, 2] and t.hdr["error"] == ref.OK
    t.step(ref.make_reports([[100, 100], [200, 200], [300, 300]]), 4)  # a third birth with a full table
    assert t.hdr["error"] == ref.TABLE_OVERFLOW and t.hdr["error_frame"] == 4 and t.hdr["frames_done"] == 4
    assert t.assoc[4][:3].tolist() == [1, 2, -1]
    before = t.table_bytes().copy()
    assert (t.step(ref.make_reports([[100, 100]]), 5) == -1).all() and np.array_equal(t.table_bytes(), before)     # sticky
    o = ref.Tracker(p)
    o.step(ref.make_reports([[1, 1]]), 0, overflow=1)
    assert o.hdr["error"] == ref.SLOT_OVERFLOW and o.hdr["error_frame"] == 0 and o.hdr["n_live"] == 0
    o = ref.Tracker(p)
    o.step(ref.make_reports([[1, 1]]), 0, count=9)
    assert o.hdr["error"] == ref.SLOT_OVERFLOW


def test_restatement_ties():
    """Power-of-two gates and integer states: every d2 is exact.  Two reports equidistant from one track: the smaller r; two
    tracks equidistant from one report: the smaller slot, and the other track coasts."""
    p = ref.params(max_tracks=4, max_detections=8, gate_az=4.0, gate_rg=4.0)
    t = ref.run([ref.make_reports([[10, 10]]), ref.make_reports([[8, 10], [12, 10]])], p)
    assert t.assoc[1][:2].tolist() == [0, -1] and t.hdr["n_live"] == 1
    t = ref.run([ref.make_reports([[10, 10], [14, 10]]), ref.make_reports([[12, 10]])], p)
    assert t.assoc[1][0] == 0 and t.slots["misses"][:2].tolist() == [0, 1] and t.slots["p_i"][:2].tolist() == [11.0, 14.0]


def test_restatement_on_the_scenario():
    """The figures the feature rests on, on the restatement alone (fp64; seed 11, 24 frames, 12 straight-line targets of at most
    1.95 pixels per frame, two pairs crossing at mid-run, detection probability 0.9, 6 uniform false alarms per 512 x 512 frame,
    default parameters: gates 4 x 4, alpha 0.5, beta 0.25, 3 of 5, 3 misses).  Measured: every target's detections lie under ONE
    id - share under its id 1.000 for all 12 - all 12 ids confirmed, no confirmed track made of false alarms only (154 births, 118
    drops), velocity error of the 12 final tracks at most 0.190 pixels per frame (mean 0.124; the measurements are rounded to the
    pixel).  Asserted: share >= 0.90 (a margin of two detections in 24 frames), velocity error <= 0.30 (1.5 x the measured
    maximum)."""
    p = ref.params()
    frames, truth = ref.scenario()
    assert len(frames) == 24
    t = ref.Tracker(p)
    confirmed = set()
    for f, fr in enumerate(frames):
        t.step(fr, f)
        confirmed |= set(t.slots["id"][t.slots["status"] == ref.CONFIRMED].tolist())
    sc = ref.score(t, frames, truth, p)
    print("share", sc["share"], "births", int(t.hdr["births_total"]), "drops", int(t.hdr["drops_total"]))
    assert t.hdr["error"] == ref.OK and t.hdr["frames_done"] == 24
    assert sc["share"].min() >= 0.90
    assert len(set(sc["main"])) == 12 and set(sc["main"]) <= confirmed               # one confirmed id per target, all different
    for k in range(12):                                                              # ... and no second confirmed id on a target
        assert {x for x in sc["ids"][k] if x >= 0} & confirmed == {sc["main"][k]}
    assert not confirmed - sc["touched"]                                             # no confirmed track of false alarms only
    live = t.slots[t.slots["status"] == ref.CONFIRMED]
    errs = []
    for k, m in enumerate(sc["main"]):
        s = live[live["id"] == m]
        assert len(s) == 1
        errs.append(np.hypot(s["v_i"][0] - truth["vel"][k][0], s["v_j"][0] - truth["vel"][k][1]))
    print("velocity error max %.3f mean %.3f" % (max(errs), np.mean(errs)))
    assert max(errs) <= 0.30


def test_unwrapping_beyond_the_ambiguity():
    """A mover at 60 m/s with v_amb = 46.6 m/s: the ATI phase wraps to 60 - 93.2 = -33.2 m/s; the track's range rate (pixels per
    frame x dr / dt, coarse) picks the branch back."""
    from sarx import track
    v_amb, dr, dt, v_true = 46.6, 2.0, 0.1, 60.0
    phase = -np.pi * v_true / v_amb                                    # GmtiReport's convention: v_los = -v_amb angle / pi
    frames = [ref.make_reports([[100, int(round(50 + f * v_true * dt / dr))]], v_phase=np.array([phase])) for f in range(16)]
    p = ref.params(max_tracks=4, max_detections=4)
    t = ref.run(frames, p)
    ij = [np.stack([fr["i"], fr["j"]], 1) for fr in frames]
    res = track.TrackResult(t.table_bytes(), np.stack(t.assoc), ij, dt, dr, v_amb)
    assert len(res.tracks) == 1 and res.tracks["confirmed"][0] and len(res.paths[0]["frames"]) == 16
    tr = res.tracks[0]
    assert abs(tr["v_los_ati_mps"] - (v_true - 2 * v_amb)) < 1e-9      # wrapped
    assert abs(tr["range_rate_mps"] - v_true) < 0.5 * v_amb            # coarse, but on the right branch
    assert abs(tr["v_los_unwrapped_mps"] - v_true) < 1e-9
    assert ref.unwrap(tr["v_los_ati_mps"], tr["range_rate_mps"], v_amb) == tr["v_los_unwrapped_mps"]
    for v in (-130.0, -47.0, 0.0, 46.0, 100.0, 200.0):                 # any branch, given a range rate within v_amb of the truth
        wrapped = (v + v_amb) % (2 * v_amb) - v_amb
        assert abs(track.unwrap_speed(wrapped, v + 0.8 * v_amb, v_amb) - v) < 1e-9
        assert abs(track.unwrap_speed(wrapped, v - 0.8 * v_amb, v_amb) - v) < 1e-9


# ---- the kernels' code object ---------------------------------------------------------------------------------------------------------
def test_track_kernels_use_no_scratch():
    """From the code object's metadata: no kernel of track.hip has a private segment."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + isa_load_waits.FLAGS + ["-I", CSRC, os.path.join(CSRC, "track.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    kernels = [m for m in meta if "track_" in m[0]]
    assert len(kernels) == 3, [m[0] for m in kernels]                   # pair, resolve, init
    for name, scratch in kernels:
        assert int(scratch) == 0, name
