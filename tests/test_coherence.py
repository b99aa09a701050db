"""CPU checks of the sliding-window coherence (include/sarx_coherence.h, csrc/coherence.hip, sarx/coherence.py): the header as C99,
the C ABI and its binding, parameter validation, the sanitizer driver of the new entry points, that no kernel of coherence.hip uses
scratch, and the NumPy restatement on its own."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coherence_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_coherence.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")


def _symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sarx_coherence.h"\nint main(void) { sarx_coherence_params p; sarx_coherence_summary s; (void)p; (void)s; '
                   'return (int)sizeof(sarx_coherence_params) - 32 + (int)sizeof(sarx_coherence_summary) - 64; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(tmp_path / "t")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0          # the stated sizes
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HDR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    from sarx import _ffi
    syms = _symbols()
    assert syms == sorted(_ffi.COHERENCE_SIGNATURES), set(syms) ^ set(_ffi.COHERENCE_SIGNATURES)
    assert syms == ["sarx_coherence_check", "sarx_coherence_pair_dev", "sarx_coherence_stack_dev", "sarx_coherence_workspace_bytes"]
    for other in (_ffi.SIGNATURES, _ffi.GMTI_SIGNATURES, _ffi.REFOCUS_SIGNATURES, _ffi.BALANCE_SIGNATURES, _ffi.TRACK_SIGNATURES):
        assert not set(syms) & set(other)
    lib = _ffi.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.sarx_version() == 206
    # argument counts of the header's declarations and of the table
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name, (_, args) in _ffi.COHERENCE_SIGNATURES.items():
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, re.S).group(1)
        assert len(decl.split(",")) == len(args), name


def test_struct_layouts():
    from sarx import _ffi
    K = importlib.import_module("sarx.coherence")
    assert C.sizeof(_ffi.CoherenceParams) == 32 and C.sizeof(_ffi.CoherenceSummary) == 64 and K.SUMMARY_DTYPE.itemsize == 64
    for name, _ in _ffi.CoherenceSummary._fields_:
        assert K.SUMMARY_DTYPE.fields[name][1] == getattr(_ffi.CoherenceSummary, name).offset, name
    assert _ffi.CoherenceParams.threshold.offset == 16 and _ffi.CoherenceSummary.sum_coh.offset == 16
    assert _ffi.COH_MAX_HALF == ref.MAX_HALF == 16
    assert re.search(r"#define\s+SARX_COH_MAX_HALF\s+16\b", open(HDR).read())


def test_check_accepts_and_refuses_what_the_header_says():
    import sarx
    from sarx import _ffi
    K = importlib.import_module("sarx.coherence")
    lib = _ffi.load()

    def rc(n_az=100, n_rg=100, **kw):
        cp = _ffi.CoherenceParams(4, 4, 0, 0, 0.5, 0.0)
        for k, v in kw.items():
            setattr(cp, k, v)
        return lib.sarx_coherence_check(C.byref(cp), n_az, n_rg)

    assert rc() == 0 and rc(ha=0, hr=0) == 0 and rc(ha=16, hr=16) == 0 and rc(1, 1, ha=16, hr=16) == 0    # a window larger than the image
    assert rc(threshold=0.0) == 0 and rc(threshold=1.5) == 0 and rc(power_floor=1e30) == 0
    for bad in (dict(ha=17), dict(hr=17), dict(ha=-1), dict(hr=-1), dict(flags=1), dict(reserved=1), dict(threshold=float("nan")),
                dict(threshold=float("inf")), dict(threshold=-0.1), dict(power_floor=float("nan")), dict(power_floor=float("inf")),
                dict(power_floor=-1.0)):
        assert rc(**bad) == -1, bad                                     # SARX_ERR_INVALID
        assert len(lib.sarx_last_error(None)) > 10
    assert rc(0, 5) == -1 and rc(5, -1) == -1 and rc((1 << 20) + 1, 5) != 0
    assert lib.sarx_coherence_check(None, 10, 10) == -1
    n = C.c_size_t(12345)
    cp = sarx.CoherenceParams(window=(4, 4)).c_params()
    assert lib.sarx_coherence_workspace_bytes(C.byref(cp), 1000, 777, C.byref(n)) == 0 and n.value % 8 == 0 and n.value > 0
    assert K.workspace_bytes(cp, 1000, 777) == n.value
    cp.ha = 99
    n.value = 12345
    assert lib.sarx_coherence_workspace_bytes(C.byref(cp), 1000, 777, C.byref(n)) == -1 and n.value == 12345
    assert lib.sarx_coherence_workspace_bytes(C.byref(cp), 1000, 777, None) == -1
    # the host's own checks
    for bad in (dict(window=(17, 0)), dict(window=(0, -1)), dict(window=3), dict(threshold=float("nan")), dict(threshold=-1.0),
                dict(power_floor=float("inf")), dict(power_floor=-1.0)):
        with pytest.raises(ValueError):
            sarx.CoherenceParams(**bad).check()
    assert sarx.CoherenceParams(window=(2, 3), threshold=0.4, power_floor=0.1).check() == (2, 3)
    img = np.zeros((8, 8), np.complex64)
    with pytest.raises(ValueError):
        sarx.coherence(img, img[:, :4])
    with pytest.raises(ValueError):
        sarx.coherence(np.zeros((8, 8)), np.zeros((8, 8)))
    with pytest.raises(ValueError):
        sarx.coherence_stack(np.zeros((3, 8, 8), np.complex64), lag=3)
    with pytest.raises(ValueError, match="window"):
        sarx.focus_ati_dpca(np.zeros((16, 16), np.complex64), np.zeros((16, 16), np.complex64), 0.031, 1e-6, 1e12, 6e8, 6000.0,
                            7500.0, 8e5, 0.0, coherence=sarx.CoherenceParams(window=(40, 1)))


def test_coherence_entry_points_under_address_and_ub_sanitizer():
    r = subprocess.run(["make", "-j8", "asan-coherence"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "coherence_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_coherence_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "coherence_asan_test.cpp")).read()
    missing = [n for n in _symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing


def test_coherence_kernels_use_no_scratch():
    """From the code object's metadata: no kernel of coherence.hip has a private segment."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + isa_load_waits.FLAGS + ["-I", CSRC, os.path.join(CSRC, "coherence.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    kernels = [m for m in meta if "coherence_" in m[0]]
    assert len(kernels) == 5, [m[0] for m in kernels]                   # the pair kernel x 4, the finish kernel
    for name, scratch in kernels:
        assert int(scratch) == 0, name


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------
def test_restatement_window_zero_is_one_where_both_samples_are_nonzero():
    a, b = ref.pair((40, 33), "patch", 5)
    r = ref.coherence(a, b, (0, 0))
    both = (a != 0) & (b != 0)
    assert both.any() and (~both).any()
    np.testing.assert_allclose(np.abs(r["g"][both]), 1.0, rtol=1e-14)
    assert (r["coh"][both] == 1.0).all() and (r["coh"][~both] == 0.0).all() and (r["g"][~both] == 0).all()


@pytest.mark.parametrize("window", [(0, 0), (2, 3), (16, 16)])
def test_restatement_scaled_copy_and_swap(window):
    a = ref.speckle((37, 29), 6)
    c = 0.5 - 2.0j                                                       # exact in complex64 products: b = c a up to one rounding
    b = (a.astype(np.complex128) * c).astype(np.complex64)
    r = ref.coherence(a, b, window)
    # a conj(b) = |a|^2 conj(c): g = conj(c) / |c| for S12 = sum a conj(b); with b as the first image g = c / |c|
    np.testing.assert_allclose(r["g"], np.conj(c) / abs(c), atol=2e-7)
    s = ref.coherence(b, a, window)
    np.testing.assert_allclose(s["g"], c / abs(c), atol=2e-7)
    np.testing.assert_allclose(s["g"], np.conj(r["g"]), rtol=1e-13, atol=1e-15)       # swapping a and b conjugates g
    w = ref.speckle((37, 29), 7)
    t, u = ref.coherence(a, w, window), ref.coherence(w, a, window)
    np.testing.assert_allclose(u["g"], np.conj(t["g"]), rtol=1e-13, atol=1e-15)
    assert np.array_equal(u["coh"], t["coh"])


def test_restatement_clipped_cell_count_at_the_corners():
    n = ref.cells(50, 40, 4, 2)
    assert n[0, 0] == n[0, -1] == n[-1, 0] == n[-1, -1] == 5 * 3 and n[25, 20] == 9 * 5 and n[0, 20] == 5 * 5 and n[25, 0] == 9 * 3
    n = ref.cells(5, 7, 16, 16)                                           # a window larger than the image
    assert (n == 35).all()
    assert ref.cells(1, 1, 16, 16)[0, 0] == 1
    a = np.ones((50, 40), np.complex64)
    r = ref.coherence(a, a, (4, 2))
    np.testing.assert_array_equal(r["s11"], ref.cells(50, 40, 4, 2))      # sums of ones count the cells


def test_restatement_change_scene():
    """96 x 80, window (4, 4), threshold 0.5: every pixel at least 6 inside the replaced patch is changed, every pixel at least 6
    outside it is unchanged."""
    a, b, (i0, j0, size) = ref.change_scene()
    r = ref.coherence(a, b, (4, 4), threshold=0.5, power_floor=0.0)
    i, j = np.mgrid[:96, :80]
    inner = (i >= i0 + 6) & (i < i0 + size - 6) & (j >= j0 + 6) & (j < j0 + size - 6)
    outer = (i < i0 - 6) | (i >= i0 + size + 6) | (j < j0 - 6) | (j >= j0 + size + 6)
    print(f"inner max coh {r['coh'][inner].max():.3f}, outer min coh {r['coh'][outer].min():.3f}")
    assert r["tested"].all()
    assert r["changed"][inner].all() and (r["mask"][inner] == 2).all()
    assert not r["changed"][outer].any() and (r["mask"][outer] == 1).all()
    assert r["coh"][inner].max() <= 0.5 and r["coh"][outer].min() >= 0.9
    assert r["n_changed"] == int((r["mask"] == 2).sum()) and r["n_tested"] == 96 * 80
    assert ref.clear_of_the_rule(r, 0.5, 0.0)
    # a power floor takes the zero patch of another scene out of the test
    a, b = ref.pair((96, 80), "patch", 9)
    r = ref.coherence(a, b, (4, 4), threshold=0.5, power_floor=0.25)
    assert (r["mask"][96 // 4 + 5:96 // 4 + 35, 80 // 5 + 5:80 // 5 + 35] == 0).all() and r["n_tested"] < 96 * 80
