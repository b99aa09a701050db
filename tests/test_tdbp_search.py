"""CPU checks of the back-projection's focus-velocity search (include/sarx_tdbp_search.h, csrc/tdbp_search.hip,
sarx/tdbp_search.py): header, binding and record layout, the line and parabola helpers, recovery of the along-track velocity
through the NumPy restatement (which fixes the scene for tests/test_gpu_tdbp_search.py), and the sanitizer driver."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tdbp_search_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_tdbp_search.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")
NAMES = ("sarx_tdbp_search_dev", "sarx_tdbp_search_host", "sarx_tdbp_search_route", "sarx_tdbp_search_set_chunks",
         "sarx_tdbp_search_metric_dev")


def _symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from sarx import _ffi
    syms = _symbols()
    assert syms == sorted(_ffi.TDBP_SEARCH_SIGNATURES) == sorted(NAMES)
    assert not set(syms) & set(_ffi.SIGNATURES)                       # sarx.h got no new function
    sarx_h = open(os.path.join(ROOT, "include", "sarx.h")).read()
    assert "tdbp_search" not in sarx_h
    text = open(HDR).read()
    assert int(re.search(r"#define SARX_TDBP_SEARCH_MAX_HYP (\d+)", text).group(1)) == _ffi.TDBP_SEARCH_MAX_HYP == ref.MAX_HYP == 1024
    assert int(re.search(r"#define SARX_TDBP_SEARCH_MAX_CHUNKS (\d+)", text).group(1)) == _ffi.TDBP_SEARCH_MAX_CHUNKS


def test_header_is_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sarx_tdbp_search.h"\nint main(void) { return sizeof(sarx_tdbp_search_record) == 32 ? 0 : 1; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_record_is_32_bytes_and_library_exports_the_symbols():
    import importlib
    import sarx
    from sarx import _ffi
    tdbp_search = importlib.import_module("sarx.tdbp_search")         # sarx.tdbp_search itself is the function of that name
    assert C.sizeof(_ffi.TdbpSearchRecord) == 32 == tdbp_search.RECORD_DTYPE.itemsize == ref.RECORD_DTYPE.itemsize
    for name, _ in _ffi.TdbpSearchRecord._fields_:
        assert tdbp_search.RECORD_DTYPE.fields[name][1] == getattr(_ffi.TdbpSearchRecord, name).offset == ref.RECORD_DTYPE.fields[name][1]
    assert _ffi.TdbpSearchRecord.peak_ix.offset == 24 and _ffi.TdbpSearchRecord.peak_iy.offset == 28
    lib = _ffi.load()
    for s in NAMES:
        assert hasattr(lib, s), s
    for name in ("tdbp_search", "tdbp_velocity_line", "tdbp_autofocus", "TdbpSearchResult"):
        assert name in sarx.__all__ and hasattr(sarx, name)


def _result(hyps, y, s2=None):
    import sarx
    rec = np.zeros(len(y), dtype=ref.RECORD_DTYPE)
    rec["s4"], rec["peak"], rec["s2"] = y, y, np.ones(len(y)) if s2 is None else s2
    return sarx.TdbpSearchResult(np.asarray(hyps, dtype=np.float64), rec, None, "tile")


def test_velocity_line():
    import sarx
    c, d = np.array([3.0, -2.0, 0.5]), np.array([3.0, 4.0, 0.0])
    got = sarx.tdbp_velocity_line(c, d, 10.0, 5)
    want = np.array([c + s * np.array([0.6, 0.8, 0.0]) for s in (-10.0, -5.0, 0.0, 5.0, 10.0)])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(got, ref.velocity_line(c, d, 10.0, 5), rtol=0, atol=1e-14)
    assert np.array_equal(got[2], c)                                  # n odd: the centre itself is a hypothesis
    assert np.array_equal(sarx.tdbp_velocity_line(c, d, 10.0, 1), c[None, :])
    for bad in (dict(n=4), dict(n=0), dict(direction=np.zeros(3)), dict(half_span=-1.0), dict(half_span=float("nan")),
                dict(direction=np.ones(2))):
        kw = dict(center=c, direction=d, half_span=10.0, n=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            sarx.tdbp_velocity_line(**kw)


@pytest.mark.parametrize("vertex", [0.0, 0.7, -1.3, 1.49, 4.4, -10.0])
def test_parabola_is_exact_on_a_sampled_parabola(vertex):
    import sarx
    s = np.arange(-4, 5) * 3.0
    hyps = sarx.tdbp_velocity_line(np.array([5.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), 12.0, 9)
    y = 100.0 - 0.37 * (s - vertex) ** 2
    for metric in ("s4", "peak", "sharpness"):
        e = _result(hyps, y).estimate(metric)
        assert not e.edge and abs(e.offset - vertex) < 1e-12 and e.index == 4 + int(np.round(vertex / 3.0))
        np.testing.assert_allclose(e.velocity, [5.0 + vertex, 1.0, 0.0], rtol=0, atol=1e-12)
    want, edge = ref.line_estimate(s, y)
    assert not edge and abs(want - vertex) < 1e-12


def test_sharpness_is_s4_over_s2_squared():
    hyps = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    r = _result(hyps, np.array([4.0, 9.0, 8.0]), s2=np.array([1.0, 3.0, 2.0]))
    np.testing.assert_array_equal(r.metric("sharpness"), np.array([4.0, 1.0, 2.0]))
    assert r.estimate("sharpness").index == 0 and r.estimate("s4").index == 1
    with pytest.raises(ValueError):
        r.estimate("entropy")


def test_edge_sets_the_flag_and_the_clip_holds():
    import sarx
    hyps = sarx.tdbp_velocity_line(np.zeros(3), np.array([0.0, 1.0, 0.0]), 4.0, 5)
    for y, idx, off in ((np.array([9.0, 5, 4, 3, 2]), 0, -4.0), (np.array([1.0, 2, 3, 4, 9]), 4, 4.0)):
        e = _result(hyps, y).estimate()
        assert e.edge and e.index == idx and e.offset == off and np.array_equal(e.velocity, hyps[idx])
        assert ref.line_estimate(np.arange(-2, 3) * 2.0, y) == (off, True)
    # around an argmax the vertex lies within half a step by itself (a = yb - y-, c = yb - y+ >= 0: (a - c) / (2 (a + c))), up to
    # rounding; the clip is what holds it there for nearly flat triples, and for any other triple
    from sarx.tdbp_search import parabola_vertex
    assert parabola_vertex(0.0, 1.0, 5.0) == -0.5 and parabola_vertex(5.0, 1.0, 0.0) == 0.5 and parabola_vertex(2.0, 2.0, 2.0) == 0.0
    for y in (np.array([0.0, 1.0, 1.0 + 1e-9, 0.0, 0.0]), np.array([0.0, 5.0, 5.0 + 1e-12, 5.0 - 3e-12, 0.0]),
              np.array([0.0, 1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 0.0])):
        e = _result(hyps, y).estimate()
        assert not e.edge and abs(e.offset - 2.0 * (e.index - 2)) <= 1.0
        assert abs(e.offset - ref.line_estimate(np.arange(-2, 3) * 2.0, y)[0]) < 1e-12
    e = _result(hyps, np.array([0.0, 7.0, 7.0, 7.0, 0.0])).estimate()
    assert e.index == 1 and not e.edge and abs(e.offset - (-2.0 + 1.0)) < 1e-12      # 1/2 (0 - 7) / (0 - 14 + 7) = +1/2 step exactly
    # a single hypothesis and a bent line
    assert _result(hyps[:1], np.array([1.0])).estimate().edge
    bent = hyps.copy()
    bent[3, 0] += 0.1
    with pytest.raises(ValueError):
        _result(bent, np.array([0.0, 1, 2, 1, 0])).estimate()
    with pytest.raises(ValueError):
        _result(hyps, np.array([0.0, 1, np.nan, 1, 0])).estimate()


def test_tie_rule_of_the_restatement():
    img = np.zeros((3, 4), np.complex128)
    img[2, 1] = img[0, 3] = 3 - 4j
    img[1, 0] = 5j                                                    # 25, like the other two: the smallest iy * nx + ix wins
    s2, s4, peak, ix, iy = ref.metrics(img)
    assert (s2, s4, peak, ix, iy) == (75.0, 3 * 625.0, 25.0, 3, 0)


@pytest.fixture(scope="module")
def recovery():
    sc = ref.recovery_scene()
    hyps = ref.recovery_hyps(sc)
    return sc, hyps, ref.records(ref.stack_images(sc, hyps, ref.RECOVERY_NX, ref.RECOVERY_NY))


def test_restatement_recovers_the_along_track_velocity(recovery):
    """DESIGN.md 4.17's curve: sum |I|^4 over nine along-track offsets from the truth is unimodal with its maximum at the truth,
    and the parabola lands within half a grid step (1.5 m/s) of it."""
    sc, hyps, rec = recovery
    print("s4:", " ".join(f"{v:.3e}" for v in rec["s4"]))
    assert int(np.argmax(rec["s4"])) == 4 and np.array_equal(hyps[4], sc["v_tgt"])
    assert (np.diff(rec["s4"][:5]) > 0).all() and (np.diff(rec["s4"][4:]) < 0).all()
    e = _result(hyps, rec["s4"]).estimate("s4")
    print("estimate:", e)
    assert not e.edge and np.linalg.norm(e.velocity - sc["v_tgt"]) < 1.5
    assert abs(ref.line_estimate(ref.RECOVERY_OFFSETS, rec["s4"])[0] - e.offset) < 1e-9


def test_tdbp_search_entry_points_under_address_and_ub_sanitizer():
    """The stand-alone driver (its own main, against libsarx_asan.so), built and run on the CPU."""
    r = subprocess.run(["make", "-j8", "asan-tdbpsearch"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "tdbpsearch_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "tdbpsearch_asan_test.cpp")).read()
    missing = [n for n in _symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing
