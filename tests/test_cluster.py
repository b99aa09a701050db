"""CPU checks of the GMTI plot extraction (include/sarx_cluster.h, csrc/cluster.hip, sarx/cluster.py): the C ABI and its binding,
the header as C99, the sanitizer driver of the new entry points, parameter validation, the restatement on an example worked by
hand, and that no kernel of cluster.hip uses scratch."""
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
import _cluster_numpy as ref  # noqa: E402

HDR = os.path.join(ROOT, "include", "sarx_cluster.h")
CSRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc")
NAMES = ("sarx_cluster_check", "sarx_cluster_plots_bytes", "sarx_cluster_step_dev", "sarx_cluster_run_dev")


def _cluster_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sarx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from sarx import _ffi
    syms = _cluster_symbols()
    assert syms == sorted(_ffi.CLUSTER_SIGNATURES) == sorted(NAMES), set(syms) ^ set(_ffi.CLUSTER_SIGNATURES)
    for other in (_ffi.SIGNATURES, _ffi.GMTI_SIGNATURES, _ffi.REFOCUS_SIGNATURES, _ffi.BALANCE_SIGNATURES, _ffi.TRACK_SIGNATURES,
                  _ffi.COHERENCE_SIGNATURES, _ffi.OSCFAR_SIGNATURES):
        assert not set(syms) & set(other)
    text = open(HDR).read()
    assert int(re.search(r"#define SARX_CLUSTER_MAX_LINK (\d+)", text).group(1)) == _ffi.CLUSTER_MAX_LINK == ref.MAX_LINK == 64
    assert int(re.search(r"#define SARX_CLUSTER_MAX_DETECTIONS (\d+)", text).group(1)) == _ffi.CLUSTER_MAX_DETECTIONS == \
        ref.MAX_DETECTIONS == 16384


def test_library_exports_the_cluster_symbols():
    import sarx
    from sarx import _ffi
    lib = _ffi.load()
    for s in _cluster_symbols():
        assert hasattr(lib, s), s
    assert lib.sarx_version() == 206                                   # sarx.h and its version stay what they were
    for name in ("gmti_cluster", "ClusterParams", "GmtiPlots"):
        assert name in sarx.__all__ and hasattr(sarx, name)


def test_struct_layouts():
    from sarx import _ffi, cluster
    assert C.sizeof(_ffi.ClusterParams) == 16 and C.sizeof(_ffi.ClusterPlot) == 64
    for dtype in (cluster.PLOT_DTYPE, ref.PLOT_DTYPE):
        assert dtype.itemsize == 64
        for name, _ in _ffi.ClusterPlot._fields_:
            assert dtype.fields[name][1] == getattr(_ffi.ClusterPlot, name).offset, name
    assert _ffi.ClusterPlot.sum_power.offset == 24 and _ffi.ClusterPlot.reserved.offset == 56
    assert cluster.PLOT_AXES_DTYPE.names[:len(cluster.PLOT_DTYPE.names)] == cluster.PLOT_DTYPE.names


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sarx_cluster.h"\nint main(void) { sarx_cluster_plot s; sarx_cluster_params p; (void)s; (void)p; '
                   'return (int)sizeof(sarx_cluster_plot) - 64 + (int)sizeof(sarx_cluster_params) - 16; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HDR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "t"                                               # ... and the sizes are what the header says
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_cluster_entry_points_under_address_and_ub_sanitizer():
    r = subprocess.run(["make", "-j8", "asan-cluster"], cwd=CSRC, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    exe = os.path.join(ROOT, "build", "asan", "cluster_asan_test")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "all checks passed" in r.stdout
    assert not re.search(r"ERROR: (Address|Leak)Sanitizer|runtime error:", r.stdout + r.stderr), (r.stdout + r.stderr)[-4000:]


def test_the_cluster_driver_calls_every_entry_point_of_its_header():
    drv = open(os.path.join(ROOT, "tests", "asan", "cluster_asan_test.cpp")).read()
    missing = [n for n in _cluster_symbols() if not re.search(r"\b" + n + r"\s*\(", drv)]
    assert not missing, missing


def test_parameter_validation():
    import sarx
    from sarx import _ffi, cluster
    for bad in (dict(link=(-1, 4)), dict(link=(4, 65)), dict(link=(65, 0)), dict(link=4), dict(link=(1, 2, 3)), dict(min_members=0)):
        with pytest.raises(ValueError):
            sarx.ClusterParams(**bad).c_params(100)
        with pytest.raises(ValueError):
            sarx.gmti_cluster(ref.make_reports([[1, 1]]), sarx.ClusterParams(**bad))
    for md in (0, 16385):
        with pytest.raises(ValueError):
            sarx.ClusterParams().c_params(md)
    with pytest.raises(ValueError, match="max_detections"):
        sarx.gmti_cluster(ref.make_reports([[1, 1]]), sarx.ClusterParams(), max_detections=16385)
    from sarx.batch import TwoChannelBatch
    with pytest.raises(ValueError, match="cluster"):
        TwoChannelBatch(None, 64, 2, stack="multilook", cluster=sarx.ClusterParams())
    with pytest.raises(ValueError, match="cluster needs detect"):
        sarx.focus_ati_dpca(None, None, 0.03, 1e-6, 1e12, 1e8, 1000.0, 100.0, 1e4, 0.0, cluster=sarx.ClusterParams())
    # the library's own check, past the host's
    lib = _ffi.load()
    cp = sarx.ClusterParams(link=(64, 64), min_members=7).c_params(16384)
    assert lib.sarx_cluster_check(C.byref(cp)) == 0
    assert cluster.plots_bytes(cp) == 64 * 16384
    cp = sarx.ClusterParams(link=(0, 0)).c_params(1)
    assert lib.sarx_cluster_check(C.byref(cp)) == 0 and cluster.plots_bytes(cp) == 64
    for field, value in (("link_az", -1), ("link_az", 65), ("link_rg", -1), ("link_rg", 65), ("min_members", 0), ("max_detections", 0),
                         ("max_detections", 16385)):
        cp = sarx.ClusterParams().c_params(100)
        setattr(cp, field, value)
        assert lib.sarx_cluster_check(C.byref(cp)) != 0, field
        assert len(lib.sarx_last_error(None)) > 10
        n = C.c_size_t(77)
        assert lib.sarx_cluster_plots_bytes(C.byref(cp), C.byref(n)) != 0 and n.value == 77
    assert lib.sarx_cluster_check(None) != 0


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------
def hand_example():
    """Nine reports, link = (2, 3), every mean 1, interf = (power, -1):

        index  (i, j)    power   component
          0    (10, 10)    5     A   an L: 0 - 1 - 2 along row 10 (range steps of 3 = link_rg), 0 - 3 - 4 down column 10
          1    (10, 13)    9     A   (azimuth steps of 2 = link_az); its ends 2 and 4 are 4 rows and 6 columns apart and
          2    (10, 16)    2     A   belong together only through the chain
          3    (12, 10)    9     A   the same power as 1: the peak is the smaller index, 1
          4    (14, 10)    4     A
          5    (30, 40)    3     B   exactly link_az = 2 rows from 6: linked
          6    (32, 40)    7     B
          7    (50, 60)    6     -   link_az + 1 = 3 rows from 8: not linked, two singletons
          8    (53, 60)    8     -

    A: 5 members, peak 1, i 10 .. 14, j 10 .. 16, sum_power 29, sum_re 29, sum_im -5, wi = 50 + 90 + 20 + 108 + 56 = 324,
       wj = 50 + 117 + 32 + 90 + 40 = 329, centroid (324 / 29, 329 / 29), max_ratio 9
    B: 2 members, peak 6, i 30 .. 32, j 40, sum_power 10, sum_re 10, sum_im -2, wi = 90 + 224 = 314, wj = 120 + 280 = 400,
       centroid (31.4, 40), max_ratio 7
    min_members = 1: four plots with peaks 1, 6, 7, 8, labels 0 0 0 0 0 1 1 2 3
    min_members = 2: the singletons go: two plots, labels 0 0 0 0 0 1 1 -1 -1"""
    ij = [[10, 10], [10, 13], [10, 16], [12, 10], [14, 10], [30, 40], [32, 40], [50, 60], [53, 60]]
    rep = ref.make_reports(ij, power=np.array([5.0, 9.0, 2.0, 9.0, 4.0, 3.0, 7.0, 6.0, 8.0]))
    rep["mean"] = 1.0
    rep["interf_re"], rep["interf_im"] = rep["power"], -1.0
    return rep


def check_hand_example(res, min_members):
    """`res`: anything with header, reports, plots, labels (the restatement's Result, or a device result in its form)."""
    n_plots = 4 if min_members == 1 else 2
    assert list(res.header) == [n_plots, 0, 0, 0]
    assert res.labels[:9].tolist() == ([0, 0, 0, 0, 0, 1, 1, 2, 3] if min_members == 1 else [0, 0, 0, 0, 0, 1, 1, -1, -1])
    assert (res.labels[9:] == -1).all()
    a, b = res.plots[0], res.plots[1]
    assert (a["n_members"], a["peak_report"], a["i_min"], a["i_max"], a["j_min"], a["j_max"]) == (5, 1, 10, 14, 10, 16)
    assert (a["sum_power"], a["centroid_i"], a["centroid_j"], a["max_ratio"]) == (29.0, 324.0 / 29.0, 329.0 / 29.0, 9.0)
    assert (b["n_members"], b["peak_report"], b["i_min"], b["i_max"], b["j_min"], b["j_max"]) == (2, 6, 30, 32, 40, 40)
    assert (b["sum_power"], b["centroid_i"], b["centroid_j"], b["max_ratio"]) == (10.0, 31.4, 40.0, 7.0)
    ra, rb = res.reports[0], res.reports[1]
    assert (ra["i"], ra["j"], ra["power"], ra["interf_re"], ra["interf_im"]) == (10, 13, 9.0, 29.0, -5.0)
    assert (rb["i"], rb["j"], rb["power"], rb["interf_re"], rb["interf_im"]) == (32, 40, 7.0, 10.0, -2.0)
    if min_members == 1:
        assert res.plots["peak_report"].tolist() == [1, 6, 7, 8] and res.plots["n_members"].tolist() == [5, 2, 1, 1]
        assert res.reports["interf_im"].tolist() == [-5.0, -2.0, -1.0, -1.0]
    assert not res.plots["reserved"].any()


@pytest.mark.parametrize("min_members", [1, 2])
def test_restatement_on_the_example_worked_by_hand(min_members):
    from sarx import cluster
    assert cluster.PLOT_DTYPE == ref.PLOT_DTYPE                        # the checker and the package speak of the same record
    rep = hand_example()
    check_hand_example(ref.cluster(rep, 2, 3, min_members, max_detections=12), min_members)
    # one link narrower in azimuth, the column of the L and the pair B fall apart
    res = ref.cluster(rep, 1, 3, 1, max_detections=12)
    assert res.labels[:9].tolist() == [0, 0, 0, 1, 2, 3, 4, 5, 6] and res.plots["n_members"].tolist() == [3, 1, 1, 1, 1, 1, 1]


def test_restatement_identity_overflow_and_order():
    rep = ref.make_reports([[i, 3 * i % 17] for i in range(50)], seed=4)
    res = ref.cluster(rep, 0, 0, 1, max_detections=64)
    assert res.reports.tobytes() == rep.tobytes() and res.labels[:len(rep)].tolist() == list(range(len(rep)))
    assert (res.plots["n_members"] == 1).all()
    np.testing.assert_allclose(res.plots["centroid_i"], rep["i"], rtol=4e-16)      # (power i) / power: two roundings
    for kw in (dict(overflow=1), dict(count=65)):
        o = ref.cluster(rep, 2, 2, 1, max_detections=64, **kw)
        assert o.header.tolist() == [kw.get("count", len(rep)), 1, 0, 0] and o.reports is None and (o.labels == -1).all()
    res = ref.cluster(rep, 3, 5, 1, max_detections=64)                 # the plot list is sorted by (i, j) like its input
    key = res.reports["i"].astype(np.int64) * 1000 + res.reports["j"]
    assert res.n_plots < len(rep) and np.all(np.diff(key) > 0) and res.plots["n_members"].sum() == len(rep)


def test_gmti_plots_decodes_a_plot_slot():
    """GmtiPlots from bytes alone (no device): the plot list through gmti.decode_slot, extents and centroids through the axes."""
    import sarx
    from sarx import cluster
    rep = hand_example()
    res = ref.cluster(rep, 2, 3, 2, max_detections=12)
    det = sarx.GmtiParams(max_detections=12)
    ra, ca = 1000.0 + 2.0 * np.arange(64), -30.0 + 0.5 * np.arange(64)
    raw = ref.slot_bytes(res.reports, 12)
    p = sarx.GmtiPlots(raw, res.plots, res.labels, 9, detect=det, range_axis=ra, cross_range=ca, wavelength_m=0.03,
                       platform_speed_mps=100.0, lag_s=1e-3)
    assert len(p) == p.n_plots == 2 and p.n_reports == 9 and p.labels.tolist() == [0, 0, 0, 0, 0, 1, 1, -1, -1]
    assert p.plots.dtype == cluster.PLOT_AXES_DTYPE and p.plots["extent_az_m"].tolist() == [2.0, 1.0]
    assert p.plots["extent_rg_m"].tolist() == [12.0, 0.0]
    np.testing.assert_allclose(p.plots["centroid_range_m"], [1000.0 + 2.0 * 329.0 / 29.0, 1080.0], rtol=1e-14)
    np.testing.assert_allclose(p.plots["centroid_cross_range_m"], [-30.0 + 0.5 * 324.0 / 29.0, -30.0 + 15.7], rtol=1e-14)
    d = p.detections.detections
    assert len(d) == 2 and d["interf"].tolist() == [29.0 - 5.0j, 10.0 - 2.0j]
    np.testing.assert_allclose(d["v_los_mps"], -0.03 * np.angle(d["interf"]) / (4.0 * np.pi * 1e-3), rtol=1e-15)
    bare = sarx.GmtiPlots(raw, res.plots, None, 9)
    assert bare.detections is None and bare.labels is None and bare.plots.dtype == cluster.PLOT_DTYPE and len(bare.reports) == 2
    with pytest.raises(sarx.GmtiOverflowError):
        sarx.GmtiPlots(ref.slot_bytes(res.reports, 12, count=40, overflow=1), res.plots, None, 40, detect=det)


# ---- the kernels' code object ---------------------------------------------------------------------------------------------------------
def test_cluster_kernels_use_no_scratch():
    """From the code object's metadata: no kernel of cluster.hip has a private segment (both forms of the one launch: keys in LDS
    and keys read from the slot)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + isa_load_waits.FLAGS + ["-I", CSRC, os.path.join(CSRC, "cluster.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    kernels = [m for m in meta if "cluster_kernel" in m[0]]
    assert len(kernels) == 2, [m[0] for m in meta]
    for name, scratch in kernels:
        assert int(scratch) == 0, name
