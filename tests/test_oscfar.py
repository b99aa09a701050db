"""CPU checks of the ordered-statistic CFAR (include/sarx_oscfar.h, csrc/oscfar.hip, sarx/gmti.py method="os"): the header as
C99, the C ABI and its binding, parameter validation, the sanitizer driver of the new entry points, the threshold factor, the
NumPy restatement on its own (tests/_oscfar_numpy.py) and what the code object says about the new kernel."""
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
import _gmti_numpy as ca_ref  # noqa: E402
import _oscfar_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_oscfar.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")


def _symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sarx_oscfar.h"\nint main(void) { sarx_oscfar_params p; (void)p; '
                   'return (int)sizeof(sarx_oscfar_params) - 40 + (int)sizeof(sarx_gmti_params) - 32; }\n')
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
    assert syms == sorted(_ffi.OSCFAR_SIGNATURES), set(syms) ^ set(_ffi.OSCFAR_SIGNATURES)
    assert syms == ["sarx_gmti_oscfar_dev", "sarx_oscfar_check"]
    for other in (_ffi.SIGNATURES, _ffi.GMTI_SIGNATURES, _ffi.REFOCUS_SIGNATURES, _ffi.BALANCE_SIGNATURES, _ffi.TRACK_SIGNATURES,
                  _ffi.COHERENCE_SIGNATURES):
        assert not set(syms) & set(other)
    lib = _ffi.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.sarx_version() == 206
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name, (_, args) in _ffi.OSCFAR_SIGNATURES.items():
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, re.S).group(1)
        assert len(decl.split(",")) == len(args), name


def test_struct_layout_and_python_parameters():
    import sarx
    from sarx import _ffi
    assert C.sizeof(_ffi.OscfarParams) == 40 and C.sizeof(_ffi.GmtiParams) == 32
    assert _ffi.OscfarParams.rank.offset == 32 and _ffi.OscfarParams.flags.offset == 36 and _ffi.OscfarParams.base.offset == 0
    # the two new fields come last: positional construction as before
    p = sarx.GmtiParams((1, 2), (3, 4), 1e-4, None, 77, 0.5)
    assert (p.method, p.os_rank, p.lag_s, p.max_detections) == ("ca", None, 0.5, 77)
    assert isinstance(p.c_params(), _ffi.GmtiParams) and p.rank() is None
    q = sarx.GmtiParams(method="os")
    cp = q.c_params()
    assert isinstance(cp, _ffi.OscfarParams) and cp.rank == 312 == ref.default_rank((2, 2), (8, 8)) and cp.flags == 0
    assert cp.base.min_train == 208 and cp.base.max_detections == 4096
    assert cp.base.alpha == pytest.approx(10.25365, rel=1e-6) and q.resolved()[5] == cp.base.alpha
    assert q.slot_bytes() == sarx.GmtiParams().slot_bytes() == 16 + 48 * 4096
    assert sarx.GmtiParams(method="os", os_rank=1).c_params().rank == 1
    assert sarx.GmtiParams(method="os", alpha=4.0).c_params().base.alpha == 4.0
    for bad in (dict(method="os", os_rank=0), dict(method="os", os_rank=417), dict(method="go"), dict(os_rank=5)):
        with pytest.raises(ValueError):
            sarx.GmtiParams(**bad).c_params()


def test_check_accepts_and_refuses_what_the_header_says():
    import sarx
    from sarx import _ffi
    lib = _ffi.load()

    def rc(rank=312, flags=0, **kw):
        cp = sarx.GmtiParams(method="os").c_params()
        cp.rank, cp.flags = rank, flags
        for k, v in kw.items():
            setattr(cp.base, k, v)
        return lib.sarx_oscfar_check(C.byref(cp))

    assert rc() == 0 and rc(1) == 0 and rc(416) == 0
    for bad in (dict(rank=0), dict(rank=-1), dict(rank=417), dict(flags=1), dict(guard_az=-1), dict(alpha=0.0), dict(alpha=float("nan")),
                dict(min_train=0), dict(max_detections=0), dict(train_az=0, train_rg=0)):
        assert rc(**bad) == -1, bad                                     # SARX_ERR_INVALID
        assert len(lib.sarx_last_error(None)) > 10
    assert rc(train_az=31) not in (0, -1)                               # SARX_ERR_UNSUPPORTED, as the CA launch refuses it
    assert lib.sarx_oscfar_check(None) == -1


def test_oscfar_entry_points_under_address_and_ub_sanitizer():
    r = subprocess.run(["make", "-j8", "asan-oscfar"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "oscfar_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_oscfar_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "oscfar_asan_test.cpp")).read()
    missing = [n for n in _symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing


# ---- the threshold factor ----------------------------------------------------------------------------------------------------------
def test_alpha_closed_form_at_one_training_cell():
    from sarx.gmti import os_cfar_alpha
    for pfa in (1e-1, 1e-3, 1e-6):
        assert os_cfar_alpha(pfa, 1, 1) == pytest.approx(1.0 / pfa - 1.0, rel=1e-12)
    for bad in ((0.0, 4, 2), (1.0, 4, 2), (1e-3, 0, 1), (1e-3, 4, 0), (1e-3, 4, 5)):
        with pytest.raises(ValueError):
            os_cfar_alpha(*bad)


@pytest.mark.parametrize("n,rank", [(416, 312), (8, 6), (4224, 1)])
def test_alpha_round_trip(n, rank):
    """pfa(os_cfar_alpha(p, n, k)) = p to 1e-12 relative, with the rate evaluated as the plain product (not the host's log form)."""
    from sarx.gmti import os_cfar_alpha, os_cfar_pfa
    for pfa in (1e-2, 1e-6, 1e-9):
        a = os_cfar_alpha(pfa, n, rank)
        assert a > 0 and abs(ref.os_pfa(a, n, rank) / pfa - 1.0) <= 1e-12
        assert abs(os_cfar_pfa(a, n, rank) / pfa - 1.0) <= 1e-12
    assert os_cfar_alpha(1e-6, 416, 312) == pytest.approx(10.25365, rel=1e-6)


def test_alpha_monte_carlo():
    """400 000 trials of 17 unit exponentials (the cell and n = 16 training cells), rank 12, design pfa 1e-2: the empirical rate
    lies within 4 binomial standard deviations of the design."""
    from sarx.gmti import os_cfar_alpha
    trials, n, rank, pfa = 400_000, 16, 12, 1e-2
    a = os_cfar_alpha(pfa, n, rank)
    x = np.random.default_rng(12).exponential(1.0, (trials, n + 1))
    level = np.partition(x[:, 1:], rank - 1, axis=1)[:, rank - 1]
    rate = np.count_nonzero(x[:, 0] > a * level) / trials
    sd = np.sqrt(pfa * (1 - pfa) / trials)
    print(f"alpha {a:.6f}, empirical rate {rate:.6f}, {(rate - pfa) / sd:+.2f} sd")
    assert abs(rate - pfa) <= 4 * sd


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------
def test_restatement_on_a_9x9_plane_worked_by_hand():
    """guard (1, 1), train (1, 1): N_full = 25 - 9 = 16, min_train 8, rank 12."""
    g, t = (1, 1), (1, 1)
    assert ref.n_full(g, t) == 16
    m = np.ones((9, 9), np.float32)
    r = ref.oscfar(m, g, t, alpha=4.0, rank=12, every_cell=True)
    nt, k = r["n_train"], r["k"]
    assert nt[4, 4] == 16 and k[4, 4] == 12                               # inside: the rank itself
    assert nt[0, 0] == 3 * 3 - 2 * 2 == 5 and not r["tested"][0, 0]       # corner: below min_train
    assert nt[1, 1] == 4 * 4 - 9 == 7 and not r["tested"][1, 1]
    assert nt[0, 4] == 3 * 5 - 2 * 3 == 9 and k[0, 4] == 7                # ceil(12 * 9 / 16) = ceil(6.75)
    assert nt[1, 4] == 4 * 5 - 9 == 11 and k[1, 4] == 9                   # ceil(8.25)
    assert nt[4, 0] == 5 * 3 - 3 * 2 == 9 and nt[8, 8] == 5
    assert k.min() >= 1 and (k <= np.maximum(nt, 1)).all()
    assert ref.effective_rank(1, 9, 16) == 1 and ref.effective_rank(16, 9, 16) == 9
    assert r["cells"] == [] and (r["count"][r["tested"]] == 0).all()      # alpha P_t = 4 > 1 everywhere
    # the strict compare: P = 4 = alpha * 1 exactly is no detection, one ulp more is
    m[4, 4] = 2.0
    r = ref.oscfar(m, g, t, alpha=4.0, rank=12, every_cell=True)
    assert r["count"][4, 4] == 0 and r["level_map"][4, 4] == 1.0 and r["cells"] == []
    m[4, 4] = np.nextafter(np.float32(2.0), np.float32(3.0))
    r = ref.oscfar(m, g, t, alpha=4.0, rank=12, every_cell=True)
    assert r["count"][4, 4] == 16 and r["cells"] == [(4, 4)] and r["level"][0] == 1.0
    assert r["power"][0] == float(m[4, 4]) ** 2
    # exactly k cells below: detected; one fewer: not.  The level is the 12th smallest training power.
    big = [(2, 2), (2, 6), (6, 2), (6, 6), (2, 4)]
    for i, j in big[:4]:
        m[i, j] = 10.0
    r = ref.oscfar(m, g, t, alpha=4.0, rank=12, every_cell=True)
    assert r["count"][4, 4] == 12 and (4, 4) in r["cells"] and r["level_map"][4, 4] == 1.0
    m[big[4]] = 10.0
    r = ref.oscfar(m, g, t, alpha=4.0, rank=12, every_cell=True)
    assert r["count"][4, 4] == 11 and (4, 4) not in r["cells"] and r["level_map"][4, 4] == 100.0
    # the peak rule's tie: of two equal neighbours the one with the smaller linear index is reported
    m = np.ones((9, 9), np.float32)
    m[4, 4] = m[4, 5] = 8.0
    r = ref.oscfar(m, g, t, alpha=4.0, rank=12, every_cell=True)
    assert r["detected"][4, 4] and r["detected"][4, 5] and r["cells"] == [(4, 4)]
    # candidates only = every cell, as far as reports go
    assert ref.oscfar(m, g, t, alpha=4.0, rank=12)["cells"] == r["cells"]


def test_masking_scene_cell_averaging_misses_what_the_ordered_statistic_reports():
    from sarx.gmti import cfar_alpha, os_cfar_alpha
    m = ref.masking_scene(20261019)
    strong = sorted(c for c, db in zip(ref.MASKING_CELLS, ref.MASKING_DB) if db == 40)
    weak = [c for c, db in zip(ref.MASKING_CELLS, ref.MASKING_DB) if db == 18]
    assert ref.n_full((2, 2), (8, 8)) == 416
    assert cfar_alpha(1e-6, 416) == pytest.approx(14.04748, rel=1e-6)
    ca = ca_ref.cfar(m, (2, 2), (8, 8), pfa=1e-6)
    assert ca["cells"] == strong
    ratios = [float(ca["ratio"][c]) for c in weak]
    print("CA ratio of the 18 dB cells:", ratios)
    assert all(0.05 < x < 0.25 for x in ratios)                           # not a near miss
    o = ref.oscfar(m, (2, 2), (8, 8), alpha=os_cfar_alpha(1e-6, 416, 312), rank=312, every_cell=True)
    assert o["cells"] == sorted(ref.MASKING_CELLS)


# ---- the code object ---------------------------------------------------------------------------------------------------------------
def test_oscfar_kernel_isa_no_scratch_and_batched_tile_fill():
    """Read off the ISA: no instantiation of the kernel has a private segment, and each issues every load of its tile fill
    ((32 + 2 HA) x (64 + 2 HR) / 256 per thread; the kernel has no other load from global memory) before its first wait on a
    load."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits as isa
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + isa.FLAGS + ["-I", CSRC, os.path.join(CSRC, "oscfar.hip"), "-o", out], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    kernels = [x for x in meta if "gmti_oscfar_kernel" in x[0]]
    assert len(kernels) == 9, [x[0] for x in kernels]
    for name, scratch in kernels:
        assert int(scratch) == 0, name
    bodies = {x.group(1): x.group(2) for x in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\s*s_endpgm", text, re.S | re.M)}
    bodies = {k: v for k, v in bodies.items() if "gmti_oscfar_kernel" in k}
    assert len(bodies) == 9
    for name, body in bodies.items():
        ha, hr = (int(x) for x in re.search(r"ILi(\d+)ELi(\d+)E", name).groups())
        k = (32 + 2 * ha) * (64 + 2 * hr) // 256
        lines = body.splitlines()
        loads = [i for i, line in enumerate(lines) if isa.LOAD.match(line)]
        first_wait = next(i for i, line in enumerate(lines) if isa.WAIT.match(line) and isa.VMC.search(line))
        assert len(loads) == k, (name, len(loads), k)
        assert all(i < first_wait for i in loads), name
