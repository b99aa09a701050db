"""CPU checks of the GMTI detector (include/sarx_gmti.h, csrc/gmti.hip, sarx/gmti.py): the C ABI and its binding, the header as C99,
the sanitizer driver of the new entry points, the threshold formula, the NumPy restatement's border counting, and the CFAR kernel's
code read off the ISA."""
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
import _gmti_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_gmti.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")


def _gmti_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from sarx import _ffi
    syms = _gmti_symbols()
    assert syms == sorted(_ffi.GMTI_SIGNATURES), set(syms) ^ set(_ffi.GMTI_SIGNATURES)
    assert not set(syms) & set(_ffi.SIGNATURES)                     # sarx.h's table is untouched


def test_library_exports_the_gmti_symbols():
    from sarx import _ffi
    lib = _ffi.load()
    for s in _gmti_symbols():
        assert hasattr(lib, s), s
    assert lib.sarx_version() == 206


def test_struct_layouts_and_slot_size():
    from sarx import _ffi, gmti
    assert C.sizeof(_ffi.GmtiReport) == 48 and C.sizeof(_ffi.GmtiHeader) == 16 and C.sizeof(_ffi.GmtiParams) == 32
    assert gmti.REPORT_DTYPE.itemsize == 48
    assert gmti.GmtiParams().slot_bytes() == 16 + 48 * 4096
    assert gmti.GmtiParams(max_detections=7).slot_bytes() == 16 + 48 * 7
    with pytest.raises(ValueError):
        gmti.GmtiParams(guard=(2, 2), train=(31, 8)).resolved()
    with pytest.raises(ValueError):
        gmti.GmtiParams(train=(0, 0)).resolved()
    with pytest.raises(_ffi.SarxError):            # the library's own check, past the host's
        p = _ffi.GmtiParams(2, 2, 8, 40, 10.0, 1, 16)
        n = C.c_size_t()
        _ffi.check(_ffi.load().sarx_gmti_slot_bytes(C.byref(p), C.byref(n)))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sarx_gmti.h"\nint main(void) { sarx_gmti_report r; sarx_gmti_params p; (void)r; (void)p; '
                   'return (int)sizeof(sarx_gmti_header) - 16; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HDR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_gmti_entry_points_under_address_and_ub_sanitizer():
    r = subprocess.run(["make", "-j8", "asan-gmti"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "gmti_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_gmti_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "gmti_asan_test.cpp")).read()
    missing = [n for n in _gmti_symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing


def test_alpha_formula():
    from sarx import gmti
    assert gmti.n_full((2, 2), (8, 8)) == 21 * 21 - 25 == 416
    assert gmti.n_full((0, 0), (1, 1)) == 8
    for pfa, n in ((1e-6, 416), (1e-3, 8), (0.5, 1), (1e-9, 928)):
        a = gmti.cfar_alpha(pfa, n)
        assert a == pytest.approx(n * (pfa ** (-1.0 / n) - 1.0), rel=1e-15)
        assert (1 + a / n) ** (-n) == pytest.approx(pfa, rel=1e-9)      # Pfa of CA-CFAR on exponential power
    assert gmti.cfar_alpha(0.5, 1) == pytest.approx(1.0)
    p = gmti.GmtiParams(pfa=1e-6)
    assert p.resolved()[5] == pytest.approx(ref.cfar_alpha(1e-6, 416), rel=1e-15)
    assert gmti.GmtiParams(alpha=7.5).resolved()[5] == 7.5
    assert p.c_params().min_train == 208


def test_reference_border_counting_on_9x9():
    """Hand-built 9 x 9 cases of the restatement: training counts at corners, edges and centre, the half-window rule, the
    threshold with an edge cell's full-window alpha, and the peak rule's tie-break."""
    guard, train = (1, 1), (2, 2)                              # outer 7 x 7 = 49, guard 9: N_full = 40
    assert ref.n_full(guard, train) == 40
    m = np.ones((9, 9), np.float32)
    r = ref.cfar(m, guard, train, alpha=2.0)
    n = r["n_train"]
    assert n[4, 4] == 40
    assert n[0, 0] == 4 * 4 - 2 * 2 == 12                     # corner: rows 0..3, cols 0..3 minus the guard rows 0..1, cols 0..1
    assert n[0, 4] == 4 * 7 - 2 * 3 == 22
    assert n[3, 3] == 7 * 7 - 9 == 40 and n[2, 2] == 6 * 6 - 9 == 27
    assert n[1, 4] == 5 * 7 - 3 * 3 == 26
    np.testing.assert_allclose(r["mean"], 1.0)                 # flat plane: the mean is 1 wherever it is taken
    assert r["cells"] == []
    tested = np.isfinite(r["ratio"])
    assert tested[4, 4] and tested[0, 4] and not tested[0, 0] and not tested[1, 1]   # 20 = N_full / 2 is the limit: 22 yes, 12 and 20 ...
    assert r["n_train"][1, 1] == 5 * 5 - 9 == 16 and not tested[1, 1]
    # a bright cell on the edge: tested with its 22 training cells and the full-window alpha
    m2 = m.copy()
    m2[0, 4] = 2.0                                             # P = 4 > 2 * 1
    r2 = ref.cfar(m2, guard, train, alpha=2.0)
    assert r2["cells"] == [(0, 4)]
    assert r2["ratio"][0, 4] == pytest.approx(2.0)
    # its neighbour one row down sees it in its guard box only: not in the training mean, and not a peak
    assert r2["mean"][1, 4] == pytest.approx(1.0)
    r3 = ref.cfar(m2, guard, train, alpha=4.0)                 # P = 4 is not > 4 * 1
    assert r3["cells"] == []
    # two equal peaks inside one guard box: the smaller linear index is reported
    m4 = m.copy()
    m4[4, 4] = m4[4, 5] = 3.0
    r4 = ref.cfar(m4, guard, train, alpha=2.0)
    assert r4["cells"] == [(4, 4)]
    m5 = m.copy()
    m5[4, 4] = m5[5, 3] = 3.0
    assert ref.cfar(m5, guard, train, alpha=2.0)["cells"] == [(4, 4)]
    # equal peaks further apart than the guard: both
    m6 = m.copy()
    m6[2, 4] = m6[6, 4] = 3.0
    assert ref.cfar(m6, guard, train, alpha=2.0)["cells"] == [(2, 4), (6, 4)]


def _cfar_kernels_asm():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits
    src = os.path.join(CSRC, "gmti.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + isa_load_waits.FLAGS + ["-I", CSRC, src, "-o", out], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    return text, isa_load_waits


def test_cfar_kernel_isa_no_scratch_and_batched_tile_fill():
    """Read off the ISA: no kernel of gmti.hip uses scratch, and each CFAR instantiation issues every load of its tile fill
    ((32 + 2 HA) x (64 + 2 HR) / 256 per thread) before its first wait on a load - a fill written with the bounds test around the
    load waits once per load."""
    text, isa = _cfar_kernels_asm()
    scratch = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert scratch and all(int(s) == 0 for s in scratch), scratch
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\s*s_endpgm", text, re.S | re.M)}
    cfar = {k: v for k, v in bodies.items() if "gmti_cfar_kernel" in k}
    assert len(cfar) == 9
    for name, body in cfar.items():
        ha, hr = (int(x) for x in re.search(r"ILi(\d+)ELi(\d+)E", name).groups())
        k = (32 + 2 * ha) * (64 + 2 * hr) // 256
        loads = [i for i, line in enumerate(body.splitlines()) if isa.LOAD.match(line)]
        first_wait = next(i for i, line in enumerate(body.splitlines()) if isa.WAIT.match(line) and isa.VMC.search(line))
        assert len(loads) == k, (name, len(loads), k)
        assert all(i < first_wait for i in loads), name
    rows = isa.census(os.path.join(CSRC, "gmti.hip"))
    for name, loads, stores, waits, waits0, serial in rows:
        if "gmti_cfar_kernel" in name:
            assert serial <= 1, (name, serial)
