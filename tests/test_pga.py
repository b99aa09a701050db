"""CPU checks of the phase-gradient autofocus (include/sarx_pga.h, csrc/pga.hip, sarx/pga.py): the header as C99, the C ABI and its
binding, what sarx_pga_check refuses, the sanitizer driver of the new entry points, that no kernel of pga.hip uses scratch, and the
NumPy restatement on its own: it recovers the injected errors of the issue, and its inputs stay clear of every discrete choice."""
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
import _pga_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_pga.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")
NAMES = ["sarx_pga_apply_dev", "sarx_pga_check", "sarx_pga_dev", "sarx_pga_workspace_bytes"]


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def _symbols():
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", _text())))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "sarx_pga.h"\nint main(void) { return (int)sizeof(sarx_pga_params) - 56 + (int)sizeof(sarx_pga_record) - 32'
                   ' + (int)offsetof(sarx_pga_params, min_contrast) - 40 + (int)offsetof(sarx_pga_record, n_cols_used) - 24; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(tmp_path / "t")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0          # the stated sizes and offsets
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HDR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_binding_and_library_agree():
    import sarx
    from sarx import _ffi
    syms = _symbols()
    assert syms == sorted(_ffi.PGA_SIGNATURES) == NAMES
    for other in (_ffi.SIGNATURES, _ffi.REFOCUS_SIGNATURES, _ffi.COHERENCE_SIGNATURES, _ffi.RELOCATE_SIGNATURES, _ffi.KTRACK_SIGNATURES):
        assert not set(syms) & set(other)
    lib = _ffi.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.sarx_version() == 206
    for name, (_, args) in _ffi.PGA_SIGNATURES.items():                  # argument counts of the header's declarations and of the table
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", _text(), re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    for name in ("pga", "apply_azimuth_phase", "PgaParams", "PgaResult"):
        assert name in sarx.__all__ and hasattr(sarx, name)


def test_struct_layouts():
    from sarx import _ffi
    K = importlib.import_module("sarx.pga")
    assert C.sizeof(_ffi.PgaParams) == 56 and C.sizeof(_ffi.PgaRecord) == 32 == K.RECORD_DTYPE.itemsize == ref.RECORD_DTYPE.itemsize
    for name, _ in _ffi.PgaRecord._fields_:
        assert K.RECORD_DTYPE.fields[name][1] == getattr(_ffi.PgaRecord, name).offset == ref.RECORD_DTYPE.fields[name][1], name
    assert (_ffi.PgaParams.n_iter.offset, _ffi.PgaParams.half_width.offset, _ffi.PgaParams.reserved.offset,
            _ffi.PgaParams.min_contrast.offset, _ffi.PgaParams.power_floor.offset) == (0, 4, 36, 40, 48)
    assert (_ffi.PgaRecord.rms_phase.offset, _ffi.PgaRecord.n_cols_used.offset, _ffi.PgaRecord.n_bins_supported.offset) == (16, 24, 28)
    text = open(HDR).read()
    assert re.search(r"#define\s+SARX_PGA_MAX_ITER\s+8\b", text) and _ffi.PGA_MAX_ITER == 8
    assert re.search(r"#define\s+SARX_PGA_MAX_FRAMES\s+65535\b", text) and _ffi.PGA_MAX_FRAMES == 65535
    assert _ffi.PGA_SIZES == ref.SIZES


def _rc(lib, n_az=256, n_rg=100, ld=None, n_frames=1, frame_stride=0, **kw):
    from sarx import _ffi
    cp = _ffi.PgaParams(3, (C.c_int32 * 8)(64, 32, 16, 0, 0, 0, 0, 0), 0, 2.0, 0.05)
    for k, v in kw.items():
        if k.startswith("h"):
            cp.half_width[int(k[1:])] = v
        else:
            setattr(cp, k, v)
    return lib.sarx_pga_check(C.byref(cp), n_az, n_rg, n_rg if ld is None else ld, n_frames, frame_stride)


def test_check_accepts_what_the_header_allows():
    from sarx import _ffi
    lib = _ffi.load()
    assert _rc(lib) == 0
    for n_az in ref.SIZES:
        assert _rc(lib, n_az=n_az, h0=(n_az - 1) // 2, h1=1, h2=1) == 0       # 2 h + 1 = L - 1 <= L
    assert _rc(lib, n_rg=1) == 0 and _rc(lib, ld=105) == 0
    assert _rc(lib, n_iter=1) == 0 and _rc(lib, n_iter=8, h3=3, h4=3, h5=3, h6=3, h7=3) == 0
    assert _rc(lib, min_contrast=0.0, power_floor=0.0) == 0 and _rc(lib, power_floor=0.999) == 0
    assert _rc(lib, h3=-5) == 0                                             # half-widths past n_iter are not looked at
    assert _rc(lib, ld=105, n_frames=3, frame_stride=255 * 105 + 100) == 0  # frames that just touch
    assert _rc(lib, n_frames=1, frame_stride=0) == 0                        # one frame: the stride is not looked at


@pytest.mark.parametrize("bad", [
    dict(n_az=100), dict(n_az=32), dict(n_az=2048), dict(n_az=0),                      # L not in the list
    dict(h0=128), dict(h2=200), dict(n_az=64, h0=32), dict(h1=0), dict(h0=-1),          # 2 h + 1 > L, h < 1
    dict(n_iter=0), dict(n_iter=9), dict(n_iter=-1),
    dict(ld=99), dict(ld=0),                                                             # ld < n_rg
    dict(n_frames=2, frame_stride=255 * 100 + 99), dict(n_frames=2, frame_stride=0),     # overlapping frames
    dict(ld=105, n_frames=3, frame_stride=255 * 105 + 99),
    dict(power_floor=1.0), dict(power_floor=-0.01), dict(power_floor=float("nan")), dict(power_floor=1.5),
    dict(min_contrast=-1.0), dict(min_contrast=float("nan")), dict(min_contrast=float("inf")),
    dict(n_rg=0), dict(n_rg=(1 << 20) + 1), dict(n_frames=0), dict(n_frames=65536), dict(reserved=1)], ids=str)
def test_check_refuses(bad):
    from sarx import _ffi
    lib = _ffi.load()
    assert _rc(lib, **bad) == -1                                           # SARX_ERR_INVALID
    assert len(lib.sarx_last_error(None)) > 10


def test_check_null_and_the_size_query():
    import sarx
    from sarx import _ffi
    K = importlib.import_module("sarx.pga")
    lib = _ffi.load()
    assert lib.sarx_pga_check(None, 256, 10, 10, 1, 0) == -1
    cp = sarx.PgaParams().c_params(512)
    assert list(cp.half_width) == [128, 64, 32, 16, 0, 0, 0, 0] and cp.n_iter == 4
    n = C.c_size_t(12345)
    assert lib.sarx_pga_workspace_bytes(C.byref(cp), 512, 512, 512, 46, 512 * 512, C.byref(n)) == 0
    assert n.value == 46 * 64 * (3 * 512 + 4) * 8 == K.workspace_bytes(cp, 512, 512, 512, 46, 512 * 512)      # 8 columns per tile at L = 512
    n.value = 12345
    assert lib.sarx_pga_workspace_bytes(C.byref(cp), 500, 512, 512, 1, 0, C.byref(n)) == -1 and n.value == 12345
    assert lib.sarx_pga_workspace_bytes(C.byref(cp), 512, 512, 512, 1, 0, None) == -1
    # the host's own checks
    assert ref.default_half_widths(64, 5) == K.default_half_widths(64, 5) == [16, 8, 4, 3, 3]
    for bad in (dict(n_iter=0), dict(n_iter=9), dict(half_widths=[3]), dict(half_widths=[300, 3, 3, 3]), dict(half_widths=[0, 3, 3, 3]),
                dict(min_contrast=-1.0), dict(min_contrast=float("nan")), dict(power_floor=1.0), dict(power_floor=-0.1)):
        with pytest.raises(ValueError):
            sarx.PgaParams(**bad).c_params(512)
    with pytest.raises(ValueError):
        sarx.PgaParams().c_params(500)


def test_pga_entry_points_under_address_and_ub_sanitizer():
    r = subprocess.run(["make", "-j8", "asan-pga"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "pga_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_pga_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "pga_asan_test.cpp")).read()
    missing = [n for n in _symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing


def test_pga_kernels_use_no_scratch():
    """From the code object's metadata: no kernel of pga.hip has a private segment."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + isa_load_waits.FLAGS + ["-I", CSRC, os.path.join(CSRC, "pga.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    kernels = [m for m in meta if "pga_" in m[0]]
    assert len(kernels) == 15, [m[0] for m in kernels]                    # estimate, integrate and apply for each of the five L
    for name, scratch in kernels:
        assert int(scratch) == 0, name


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------
def test_restatement_apply_is_exact_and_reversible():
    img = ref.scene(64, 5, 2, 3)
    phi = ref.error("cubic_sine", 64)
    there = ref.apply(img, phi, +1)
    np.testing.assert_allclose(ref.apply(there, phi, -1), img, atol=1e-12)
    # a linear phase over k is a circular shift along azimuth: bin u = (k - L/2) mod L, so phi = -2 pi (k - L/2) / L shifts by one row
    k = np.arange(64)
    shifted = ref.apply(img, -2.0 * np.pi * (k - 32) / 64.0, +1)
    np.testing.assert_allclose(shifted, np.roll(img, 1, axis=0), atol=1e-5)


def test_restatement_of_a_clean_point_is_zero_phase():
    img = np.zeros((128, 3), np.complex64)
    img[40, 1] = 3.0 - 1.0j
    e = ref.estimate(img, 16, 0.0, 0.0)
    assert e["n_cols_used"] == 1 and e["n_bins_supported"] == 128 and e["rows"][1] == 40
    assert np.abs(e["phi"]).max() < 1e-12 and e["rms_phase"] < 1e-12
    assert e["s2"] == pytest.approx(10.0) and e["s4"] == pytest.approx(100.0)
    z = ref.estimate(np.zeros((64, 4), np.complex64), 8, 0.0, 0.0)
    assert z["n_cols_used"] == 0 and z["n_bins_supported"] == 0 and not z["phi"].any() and z["rms_phase"] == 0.0


@pytest.mark.parametrize("shape,kind,min_contrast", ref.FULL_CASES, ids=[ref.case_id(*c) for c in ref.FULL_CASES])
def test_restatement_recovers_the_injected_error(shape, kind, min_contrast):
    """Measured with this restatement: residual rms 0.05 - 0.13 rad, output sharpness >= the unblurred scene's in every case.  The
    rms is noise-limited at 30 dB, it is not an implementation tolerance."""
    c = ref.case(shape, kind, min_contrast)
    g = c["guards"]
    print(f"guards: runner-up {g['runner_up']:.6f}, contrast margin {g['contrast']:.4f}, wrap margin {g['wrap']:.3f}")
    assert ref.guards_hold(g), g                                          # a choice the fp32 kernel could flip is the input's fault
    rms = float(np.sqrt((ref.remove_line(c["phi"] - c["err"]) ** 2).mean()))
    s_out, s_clean, s_blur = ref.sharpness(c["out"]), ref.sharpness(c["clean"]), ref.sharpness(c["blur"])
    print(f"residual rms {rms:.4f} rad; sharpness out {s_out:.5g}, unblurred {s_clean:.5g}, blurred {s_blur:.5g}; "
          f"rms_phase per estimate {np.round(c['records']['rms_phase'], 4)}")
    assert rms <= 0.2
    assert s_out >= 0.98 * s_clean
    rec = c["records"]
    assert (rec["n_bins_supported"] == shape[0]).all()                    # floor 0: every bin
    if min_contrast == 0.0:
        assert (rec["n_cols_used"] == shape[1]).all()                     # every column
    else:
        assert rec["n_cols_used"][-1] == shape[2] and (rec["n_cols_used"] <= shape[2]).all()      # the targets' columns, once focused
    np.testing.assert_allclose(rec["s2"], rec["s2"][0], rtol=1e-6)        # a phase-only filter keeps the energy
    assert rec["s4"][-1] / rec["s2"][-1] ** 2 == pytest.approx(s_out, rel=1e-12)


@pytest.mark.parametrize("shape,kind", ref.BAND_CASES, ids=[ref.case_id(*c) for c in ref.BAND_CASES])
def test_restatement_band_limited(shape, kind):
    """The spectrum zeroed outside the central 40 % of the bins, floor 0.05 (inside the leakage).  Measured: in-band residual rms
    0.05 - 0.12 rad."""
    c = ref.case(shape, kind, 0.0, band=True)
    g = c["guards"]
    print(f"guards: runner-up {g['runner_up']:.6f}, floor margin {g['floor']:.4f}, wrap margin {g['wrap']:.3f}")
    assert ref.guards_hold(g), g
    band = c["band"]
    res = ref.remove_line(c["phi"] - c["err"], band)
    rms = float(np.sqrt((res[band] ** 2).mean()))
    s_out, s_blur = ref.sharpness(c["out"]), ref.sharpness(c["blur"])
    print(f"in-band residual rms {rms:.4f} rad; sharpness out {s_out:.5g}, blurred {s_blur:.5g}; bins supported {c['records']['n_bins_supported']} "
          f"of {int(band.sum())} in band")
    assert rms <= 0.2
    assert s_out > s_blur
    assert (c["records"]["n_bins_supported"] < shape[0]).all() and (c["records"]["n_bins_supported"] >= band.sum()).all()


@pytest.mark.parametrize("shape,kind,min_contrast", ref.EXTRA_CASES, ids=[ref.case_id(*c) for c in ref.EXTRA_CASES])
def test_the_gpu_tests_further_inputs_are_guarded_too(shape, kind, min_contrast):
    assert ref.guards_hold(ref.case(shape, kind, min_contrast)["guards"])
