"""CPU checks of the two-channel balance (include/sarx_balance.h, csrc/balance.hip, sarx/balance.py): the C ABI and its binding,
the header as C99, the sanitizer driver of the new entry points, parameter validation, the NumPy restatement on its own, and that
no kernel of balance.hip uses scratch."""
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
import _balance_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_balance.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")


def _balance_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from sarx import _ffi
    syms = _balance_symbols()
    assert syms == sorted(_ffi.BALANCE_SIGNATURES), set(syms) ^ set(_ffi.BALANCE_SIGNATURES)
    for other in (_ffi.SIGNATURES, _ffi.GMTI_SIGNATURES, _ffi.REFOCUS_SIGNATURES):
        assert not set(syms) & set(other)
    for name in ("sarx_balance_table_bytes", "sarx_balance_workspace_bytes", "sarx_balance_estimate_dev", "sarx_balance_apply_dev"):
        assert name in syms


def test_library_exports_the_balance_symbols():
    from sarx import _ffi
    lib = _ffi.load()
    for s in _balance_symbols():
        assert hasattr(lib, s), s
    assert lib.sarx_version() == 206


def test_struct_layouts():
    from sarx import _ffi, balance
    assert C.sizeof(_ffi.BalanceHeader) == 64 and C.sizeof(_ffi.BalanceRecord) == 64 and C.sizeof(_ffi.BalanceParams) == 40
    for struct, dtype in ((_ffi.BalanceHeader, balance.HEADER_DTYPE), (_ffi.BalanceRecord, balance.RECORD_DTYPE)):
        assert dtype.itemsize == 64
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name
    assert _ffi.BalanceHeader.w_re.offset == 16 and _ffi.BalanceRecord.coherence.offset == 48


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sarx_balance.h"\nint main(void) { sarx_balance_record r; sarx_balance_header h; sarx_balance_params p; '
                   '(void)r; (void)h; (void)p; return (int)sizeof(sarx_balance_record) - 64 + (int)sizeof(sarx_balance_header) - 64 + '
                   '(int)sizeof(sarx_balance_params) - 40; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HDR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_balance_entry_points_under_address_and_ub_sanitizer():
    r = subprocess.run(["make", "-j8", "asan-balance"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "balance_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_balance_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "balance_asan_test.cpp")).read()
    missing = [n for n in _balance_symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing


def test_parameter_validation():
    import sarx
    from sarx import _ffi, balance
    img = np.zeros((64, 1024), np.complex64)                           # [N_rg x N_az]
    for bad in (dict(block=(7, 64)), dict(block=(64, 4097)), dict(block=(8, 8)), dict(block=64), dict(mode="lsq"),
                dict(interp="cubic"), dict(clip_db=float("nan")), dict(min_count=0), dict(min_coherence=1.5), dict(min_coherence=-0.1)):
        p = sarx.BalanceParams(**bad)
        if bad == dict(block=(8, 8)):                                  # too many blocks for this size only
            with pytest.raises(ValueError, match="blocks"):
                p.resolved(4096, 4096)
            continue
        with pytest.raises(ValueError):
            sarx.channel_balance(img, img, p)
    with pytest.raises(ValueError):
        sarx.channel_balance(img, img[:, :100])
    with pytest.raises(ValueError):
        sarx.channel_balance(np.zeros((64, 64)), np.zeros((64, 64)))    # not complex
    with pytest.raises(ValueError, match="block"):
        sarx.focus_ati_dpca(np.zeros((16, 16), np.complex64), np.zeros((16, 16), np.complex64), 0.031, 1e-6, 1e12, 6e8, 6000.0,
                            7500.0, 8e5, 0.0, balance=sarx.BalanceParams(block=(4, 4)))
    # defaults: a quarter of a full block, of the image where the block is larger
    assert sarx.BalanceParams().resolved(8192, 8192) == (256, 256, _ffi.BALANCE_LS, _ffi.BALANCE_BILINEAR, 16384)
    assert sarx.BalanceParams(block=(4096, 4096), mode="phase", interp="nearest").resolved(64, 100) == \
        (4096, 4096, _ffi.BALANCE_PHASE, _ffi.BALANCE_NEAREST, 1600)
    # the library's own check, past the host's
    lib = _ffi.load()
    cp = sarx.BalanceParams().c_params(1000, 777)
    assert lib.sarx_balance_check(C.byref(cp), 1000, 777) == 0
    assert balance.table_bytes(cp, 1000, 777) == 64 + 64 * 16
    assert balance.workspace_bytes(cp, 1000, 777) == 16 * 8 * 40
    cp.block_rg = 5000
    assert lib.sarx_balance_check(C.byref(cp), 1000, 777) != 0
    assert b"block" in lib.sarx_last_error(None)


def test_decode_and_coherence_at():
    from sarx import balance
    raw = np.zeros(64 + 64 * 6, np.uint8)
    hdr = raw[:64].view(balance.HEADER_DTYPE)
    hdr["nb_az"], hdr["nb_rg"], hdr["n_valid"], hdr["w_re"], hdr["w_im"], hdr["coherence"] = 2, 3, 5, 0.5, -0.5, 0.9
    rec = raw[64:].view(balance.RECORD_DTYPE)
    rec["w_re"], rec["w_im"] = np.arange(6.0), -np.arange(6.0)
    rec["coherence"], rec["n"], rec["valid"] = np.linspace(0.5, 1.0, 6), 100, [1, 1, 0, 1, 1, 1]
    cb = balance.ChannelBalance(raw, (32, 48), (16, 16), "bilinear", np.inf)
    assert cb.weights.shape == (2, 3) and cb.weights[1, 2] == 5 - 5j and cb.global_weight == 0.5 - 0.5j
    assert cb.valid.tolist() == [[True, True, False], [True, True, True]] and cb.counts.sum() == 600 and cb.n_valid == 5
    np.testing.assert_allclose(cb.coherence_at(7.5, 7.5), 0.5)                      # a block centre
    np.testing.assert_allclose(cb.coherence_at(15.5, 7.5), 0.5 * (0.5 + 0.8))       # half way to the block below
    np.testing.assert_allclose(cb.coherence_at(0, 47), cb.coherence[0, 2])          # constant past the outermost centres
    near = balance.ChannelBalance(raw, (32, 48), (16, 16), "nearest", np.inf)
    np.testing.assert_allclose(near.coherence_at(np.array([15, 16]), np.array([31, 32])), [near.coherence[0, 1], near.coherence[1, 2]])
    with pytest.raises(IndexError):
        cb.coherence_at(32, 0)


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------
def _noise(shape, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_restatement_recovers_a_constant_mismatch(interp):
    """slc2 = slc1 / w0 exactly (fp64 inputs of the restatement are the complex64 images): every block's LS weight is w0."""
    w0 = 0.8 * np.exp(0.7j)
    s2 = _noise((100, 77), 1)
    s1 = s2.astype(np.complex128) * w0
    # the restatement takes complex64 images: compare on images it can hold exactly
    s1c = s1.astype(np.complex64)
    t = ref.balance(s1c, s2, (32, 16), "ls", interp)
    w_exact = np.array([[np.sum(s1c[a:a + 32, r:r + 16].astype(np.complex128) * np.conj(s2[a:a + 32, r:r + 16].astype(np.complex128))) /
                         np.sum(np.abs(s2[a:a + 32, r:r + 16].astype(np.complex128)) ** 2) for r in range(0, 77, 16)] for a in range(0, 100, 32)])
    np.testing.assert_allclose(t["w"], w_exact, rtol=1e-12)
    np.testing.assert_allclose(t["w"], w0, rtol=1e-6)                   # what complex64 rounding of slc1 leaves
    # a mismatch that complex64 holds exactly (s1 = 0.5j s2) is recovered to fp64 rounding
    s1e = (s2.astype(np.complex128) * 0.5j).astype(np.complex64)
    assert np.array_equal(s1e.astype(np.complex128), s2.astype(np.complex128) * 0.5j)
    t = ref.balance(s1e, s2, (32, 16), "ls", interp)
    np.testing.assert_allclose(t["w"], 0.5j, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(t["w_pixel"], 0.5j, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(t["slc2"], s1e, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(t["coherence"], 1.0, rtol=1e-12)
    assert t["valid"].all() and t["n"].sum() == 100 * 77 and abs(t["global_weight"] - 0.5j) < 1e-12


def test_restatement_whole_image_phase_is_the_viewers_balance():
    s1, s2 = _noise((90, 50), 2), _noise((90, 50), 3)
    s1 = (s1 + 2 * s2 * np.exp(0.4j)).astype(np.complex64)
    t = ref.balance(s1, s2, (4096, 4096), "phase", "bilinear")
    total = np.sum(s1.astype(np.complex128) * np.conj(s2.astype(np.complex128)))
    assert t["w"].shape == (1, 1) and abs(abs(t["w"][0, 0]) - 1) < 1e-14
    assert np.angle(t["w"][0, 0]) == pytest.approx(np.angle(total), abs=1e-14)
    np.testing.assert_allclose(t["slc2"], s2.astype(np.complex128) * np.exp(1j * np.angle(total)), rtol=1e-12)


def test_restatement_bilinear_weight_is_linear_between_the_outermost_centres():
    nba, nbr, ba, br = 5, 4, 16, 24
    n_az, n_rg = nba * ba - 5, nbr * br - 7                            # ragged last blocks keep their nominal centre
    table = (1.0 + 0.25 * np.arange(nba)[:, None] - 0.5 * np.arange(nbr)[None, :]) + 1j * (0.1 * np.arange(nba)[:, None] + 0.3 * np.arange(nbr)[None, :])
    w = ref.interpolate(table, (n_az, n_rg), (ba, br))
    ta = np.clip((np.arange(n_az) + 0.5) / ba - 0.5, 0, nba - 1)[:, None]
    tr = np.clip((np.arange(n_rg) + 0.5) / br - 0.5, 0, nbr - 1)[None, :]
    np.testing.assert_allclose(w, (1.0 + 0.25 * ta - 0.5 * tr) + 1j * (0.1 * ta + 0.3 * tr), rtol=1e-13)
    assert w[0, 0] == table[0, 0] and w[ba // 2 - 1, 0] == table[0, 0]   # constant outside the outermost centres
    np.testing.assert_array_equal(ref.interpolate(table, (n_az, n_rg), (ba, br), "nearest")[ba, br], table[1, 1])
    one = ref.interpolate(table[:1, :1], (7, 9), (16, 24))
    assert (one == table[0, 0]).all()


def test_restatement_clip_and_validity():
    s1, s2 = _noise((64, 64), 4), _noise((64, 64), 5)
    s1[5, 5] = 100.0
    s2[32:48, 16:32] = 0                                                 # an all-zero block
    t = ref.estimate(s1, s2, (16, 16), "ls", clip_power=50.0, min_count=200)
    assert t["n"][0, 0] == 255 and t["n"][1, 1] == 256
    assert not t["valid"][2, 1] and t["valid"].sum() == 15 and t["n_valid"] == 15
    assert t["w"][2, 1] == t["global_weight"] and t["coherence"][2, 1] == 0.0
    few = ref.estimate(s1, s2, (16, 16), "ls", clip_power=50.0, min_count=256)
    assert not few["valid"][0, 0] and few["w"][0, 0] == few["global_weight"]
    none = ref.estimate(s1 * 0, s2, (16, 16))
    assert none["n_valid"] == 0 and none["global_weight"] == 1.0 and (none["w"] == 1.0).all()


def test_restatement_on_the_mismatch_fixture():
    """The figures the feature rests on, on the restatement alone (fp64, seed 7): block-adaptive balance leaves the clutter at least
    12 dB below what one least-squares weight leaves, the movers keep their DPCA power to 1 dB, and without the clip the first
    mover loses more than 1 dB."""
    s1, s2 = ref.mismatch_fixture()
    glob = ref.balance(s1, s2, (4096, 4096), "ls", "nearest", ref.FIXTURE_CLIP)
    blk = ref.balance(s1, s2, ref.FIXTURE_BLOCK, "ls", "bilinear", ref.FIXTURE_CLIP, min_count=256)
    r_glob, r_blk = ref.residue_db(s1, glob["slc2"]), ref.residue_db(s1, blk["slc2"])
    print(f"residue: global LS {r_glob:.2f} dB, block-adaptive {r_blk:.2f} dB")
    assert r_glob - r_blk >= 12.0
    want = [ref.mover_expected_db(p) for _, p in ref.FIXTURE_MOVERS]
    got = ref.mover_db(s1, blk["slc2"])
    assert np.all(np.abs(np.array(got) - want) <= 1.0), (got, want)
    noclip = ref.balance(s1, s2, ref.FIXTURE_BLOCK, "ls", "bilinear", np.inf, min_count=256)
    assert want[0] - ref.mover_db(s1, noclip["slc2"])[0] > 1.0


# ---- the kernels' code object ---------------------------------------------------------------------------------------------------------
def test_balance_kernels_use_no_scratch():
    """From the code object's metadata: no kernel of balance.hip has a private segment."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + isa_load_waits.FLAGS + ["-I", CSRC, os.path.join(CSRC, "balance.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    kernels = [m for m in meta if "balance_" in m[0]]
    assert len(kernels) == 7, [m[0] for m in kernels]                   # estimate x 2, weights, apply x 4
    for name, scratch in kernels:
        assert int(scratch) == 0, name
